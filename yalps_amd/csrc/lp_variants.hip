// lp_variants.hip -- libyalps_lpvar.so: many variants of one LP in one call (include/yalps_lpvar.h)
// C ABI, host side and the lp_variants_kernel instantiations.  A library of its own: nothing here is linked into the other
// three, and the pivot loop is libyalps_hip.so's wg_simplex.cuh, included unchanged.  The host side follows
// lp_batch_host.inc (same size classes, same pass / rerun protocol) but is not that text: one shape per call means one
// class, one image and at most two launches per pass, and including it would compile lp_batch_kernel into this library.
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

#include "../../include/yalps_lpvar.h"

#pragma clang fp contract(off)

namespace {
#include "common.cuh"

#include "wg_simplex.cuh"
#include "lp_variants_kernel.cuh"

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return fail(e_ == hipErrorOutOfMemory ? YALPS_E_NOMEM : YALPS_E_DEVICE,                         \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                                 \
    } while (0)

// ---- size classes: lp_batch_host.inc's table (LDS bytes, lanes, workgroups per CU; class 4 is the HBM form) ----
struct SizeClass {
    size_t lds_max;
    int lanes, per_cu;
};
constexpr int NCLASS = 5, HBM_CLASS = NCLASS - 1;
const SizeClass kClasses[NCLASS] = {{19 * 1024, 256, 8}, {39 * 1024, 256, 4}, {79 * 1024, 256, 2}, {SMALL_LDS_MAX, 1024, 1},
                                    {0, 1024, 1}};
constexpr size_t AUX_LDS_MAX = 64 * 1024; // HBM form: colbuf + prow stay in LDS up to this size, else behind the tableau in HBM
constexpr long long HIST_FIRST = 4096;    // first checkCycles history capacity per workgroup (YALPS_LPVAR_HIST)

int lp_class(int64_t w, int64_t h) {
    if (w < 1 || h < 1 || 8 * w * h > YALPS_LPVAR_MAX_BYTES) return -1;
    const size_t bytes = small_lds_bytes((int)w, (int)h);
    for (int k = 0; k < HBM_CLASS; k++)
        if (bytes <= kClasses[k].lds_max) return k;
    return HBM_CLASS;
}
bool lp_aux_hbm(int64_t w, int64_t h) { return sizeof(double) * ((size_t)small_pcols((int)w - 1) + (size_t)h) > AUX_LDS_MAX; }

using KernelFn = void (*)(VarLaunch);
struct KernelForm {
    KernelFn fn;
    int lanes;
    bool check, lds;
};
const KernelForm kForms[] = {
    {lp_variants_kernel<256, false, true>, 256, false, true},    {lp_variants_kernel<256, true, true>, 256, true, true},
    {lp_variants_kernel<1024, false, true>, 1024, false, true},  {lp_variants_kernel<1024, true, true>, 1024, true, true},
    {lp_variants_kernel<1024, false, false>, 1024, false, false}, {lp_variants_kernel<1024, true, false>, 1024, true, false},
};
const KernelForm *find_form(int lanes, bool check, bool lds) {
    for (const KernelForm &f : kForms)
        if (f.lanes == lanes && f.check == check && f.lds == lds) return &f;
    return nullptr;
}
std::string form_name(const KernelForm &f) {
    return "lp_variants_kernel<" + std::to_string(f.lanes) + (f.check ? ",check" : "") + (f.lds ? ",lds" : "") + ">";
}

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

int env_int(const char *name, int dflt) {
    const char *v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}
} // namespace

struct yalps_lpvar {
    int device = 0, num_cus = 256;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evb0 = nullptr, evb1 = nullptr; // a pass | the image's assembly
    long long hist_first = HIST_FIRST;
    int per_cu[NCLASS];
    DevBuf desc, order, counters, brow, bcol, bval, image, prow, pcol, pval, status, result, pivots, col0, pos, var, tab, ws, hist;
    // the last solve
    int32_t w = 0, h = 0, count = 0;
    std::vector<double> h_col0;
    std::vector<int32_t> h_pos, h_var, h_status;
    bool keep = false;
    std::string info;
};

namespace {
int ensure(DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    if (b.p) HIP_TRY(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    const size_t want = std::max(bytes, (size_t)4096);
    HIP_TRY(hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}

// cells [lo, hi) of row / col: inside the w x h tableau and strictly increasing by (row, col); 0, 1 = outside, 2 = order
int check_cells(const int32_t *row, const int32_t *col, int64_t lo, int64_t hi, int64_t w, int64_t h, int64_t *at) {
    int64_t last = -1;
    for (int64_t c = lo; c < hi; c++) {
        *at = c - lo;
        if (row[c] < 0 || row[c] >= h || col[c] < 0 || col[c] >= w) return 1;
        const int64_t key = (int64_t)row[c] * w + col[c];
        if (key <= last) return 2;
        last = key;
    }
    return 0;
}

int validate(int64_t w, int64_t h, int64_t ncells, const int32_t *brow, const int32_t *bcol, int32_t count, const int64_t *off,
             const int32_t *prow, const int32_t *pcol) {
    if (w < 1 || h < 1) return fail(YALPS_E_ARG, "yalps_lpvar: width and height must be at least 1");
    if (8 * w * h > YALPS_LPVAR_MAX_BYTES)
        return fail(YALPS_E_ARG, "yalps_lpvar: tableau of " + std::to_string(8 * w * h) + " bytes is above the limit of " +
                                     std::to_string((long long)YALPS_LPVAR_MAX_BYTES));
    if (ncells < 0) return fail(YALPS_E_ARG, "yalps_lpvar: base_cells < 0");
    if (ncells > 0 && (!brow || !bcol)) return fail(YALPS_E_ARG, "yalps_lpvar: base_row / base_col is NULL");
    int64_t at = 0;
    if (int bad = check_cells(brow, bcol, 0, ncells, w, h, &at))
        return fail(YALPS_E_ARG, bad == 1 ? "yalps_lpvar: base cell " + std::to_string(at) + " lies outside the tableau"
                                          : "yalps_lpvar: base cells are not sorted by (row, col), strictly increasing");
    if (count < 0) return fail(YALPS_E_ARG, "yalps_lpvar: count < 0");
    if (count == 0) return 0;
    if (!off) return fail(YALPS_E_ARG, "yalps_lpvar: patch_offsets is NULL");
    if (off[0] < 0) return fail(YALPS_E_ARG, "yalps_lpvar: variant 0: negative patch offset");
    for (int32_t i = 0; i < count; i++) {
        const std::string who = "yalps_lpvar: variant " + std::to_string(i) + ": ";
        if (off[i + 1] < off[i]) return fail(YALPS_E_ARG, who + "patch offsets decrease");
        if (off[i + 1] > off[i] && (!prow || !pcol)) return fail(YALPS_E_ARG, who + "patch_row / patch_col is NULL");
        if (int bad = check_cells(prow, pcol, off[i], off[i + 1], w, h, &at))
            return fail(YALPS_E_ARG, bad == 1 ? who + "patch cell " + std::to_string(at) + " lies outside the tableau"
                                              : who + "patch cells are not sorted by (row, col), strictly increasing");
    }
    return 0;
}

struct Launch {
    bool check;
    std::vector<int32_t> vars;
    const KernelForm *form;
    int grid;
};

// what a call's one shape fixes for every launch
struct Shape {
    int cls;
    bool lds, aux;
    int pitch;
    size_t image_doubles, shmem, stride; // stride: HBM form, doubles of workspace per workgroup
};

Shape shape_of(int w, int h) {
    Shape s{};
    s.cls = lp_class(w, h);
    s.lds = s.cls != HBM_CLASS;
    const int n = w - 1;
    s.pitch = s.lds ? small_lds_pitch(n) : small_pcols(n);
    s.image_doubles = (size_t)h * s.pitch + (((size_t)h + 1) & ~(size_t)1);
    if (s.lds) {
        s.shmem = small_lds_bytes(w, h);
    } else {
        const size_t lp = (size_t)small_pcols(n), aux = lp + (size_t)h;
        s.aux = lp_aux_hbm(w, h);
        if (!s.aux) s.shmem = sizeof(double) * aux;
        s.stride = (size_t)h * lp + ((aux + 1) & ~(size_t)1);
    }
    s.shmem = std::max<size_t>((s.shmem + 15) & ~(size_t)15, 16);
    return s;
}

// One pass: at most two launches (checkCycles off, on) over `todo`, enqueued before one wait.  Leaves every variant's status in h_status.
int run_pass(yalps_lpvar *b, const Shape &S, const std::vector<int32_t> &todo, const int32_t *check, long long hist_cap,
             std::vector<Launch> &launches, float *ms_out) {
    hipStream_t s = b->stream;
    launches.clear();
    for (int c = 0; c < 2; c++) {
        Launch L{c != 0, {}, nullptr, 0};
        for (int32_t i : todo)
            if ((check[i] != 0) == L.check) L.vars.push_back(i);
        if (!L.vars.empty()) launches.push_back(std::move(L));
    }
    if (launches.empty()) return 0;
    size_t order_total = 0, max_grid = 0, hist_wgs = 0;
    for (Launch &L : launches) {
        L.form = find_form(kClasses[S.cls].lanes, L.check, S.lds);
        if (!L.form) return fail(YALPS_E_ARG, "yalps_lpvar: no kernel for class " + std::to_string(S.cls));
        L.grid = (int)std::min<size_t>(L.vars.size(), (size_t)b->num_cus * (size_t)std::max(1, b->per_cu[S.cls]));
        max_grid = std::max(max_grid, (size_t)L.grid);
        if (L.check) hist_wgs = (size_t)L.grid;
        order_total += L.vars.size();
    }
    // (launches of one stream run one after the other: they share the workspace and the history pool)
    if (int rc = ensure(b->order, sizeof(int32_t) * order_total)) return rc;
    if (int rc = ensure(b->counters, sizeof(unsigned int) * launches.size())) return rc;
    if (int rc = ensure(b->ws, sizeof(double) * S.stride * max_grid)) return rc;
    if (int rc = ensure(b->hist, sizeof(int32_t) * 2 * hist_wgs * (size_t)hist_cap)) return rc;
    std::vector<int32_t> order;
    order.reserve(order_total);
    for (const Launch &L : launches) order.insert(order.end(), L.vars.begin(), L.vars.end());
    HIP_TRY(hipMemcpyAsync(b->order.p, order.data(), sizeof(int32_t) * order_total, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(b->counters.p, 0, sizeof(unsigned int) * launches.size(), s));
    HIP_TRY(hipEventRecord(b->ev0, s));
    size_t at = 0, nl = 0;
    for (const Launch &L : launches) {
        VarLaunch a{};
        a.desc = static_cast<const VarDesc *>(b->desc.p);
        a.order = static_cast<const int32_t *>(b->order.p) + at;
        a.count = (int32_t)L.vars.size();
        a.counter = static_cast<unsigned int *>(b->counters.p) + nl;
        a.w = b->w;
        a.h = b->h;
        a.aux_hbm = S.aux ? 1 : 0;
        a.image = static_cast<const double *>(b->image.p);
        a.prow = static_cast<const int32_t *>(b->prow.p);
        a.pcol = static_cast<const int32_t *>(b->pcol.p);
        a.pval = static_cast<const double *>(b->pval.p);
        a.status = static_cast<int32_t *>(b->status.p);
        a.result = static_cast<double *>(b->result.p);
        a.pivots = static_cast<long long *>(b->pivots.p);
        a.col0 = static_cast<double *>(b->col0.p);
        a.pos = static_cast<int32_t *>(b->pos.p);
        a.var = static_cast<int32_t *>(b->var.p);
        a.tab = b->keep ? static_cast<double *>(b->tab.p) : nullptr;
        a.ws = static_cast<double *>(b->ws.p);
        a.ws_stride = (long long)S.stride;
        a.hist = static_cast<int32_t *>(b->hist.p);
        a.hist_cap = hist_cap;
        const KernelFn fn = L.form->fn;
        fn<<<dim3(L.grid), dim3(L.form->lanes), S.shmem, s>>>(a);
        HIP_TRY(hipGetLastError());
        at += L.vars.size();
        nl++;
    }
    HIP_TRY(hipEventRecord(b->ev1, s));
    HIP_TRY(hipMemcpyAsync(b->h_status.data(), b->status.p, sizeof(int32_t) * (size_t)b->count, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    *ms_out += ms;
    return 0;
}

int create_impl(int32_t device, void *hip_stream, yalps_lpvar **out) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(YALPS_E_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(YALPS_E_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(YALPS_E_DEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only");
    yalps_lpvar *b = new yalps_lpvar();
    *out = b;
    b->device = device;
    b->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hip_stream) {
        b->stream = static_cast<hipStream_t>(hip_stream);
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        b->own_stream = true;
    }
    HIP_TRY(hipEventCreate(&b->ev0));
    HIP_TRY(hipEventCreate(&b->ev1));
    HIP_TRY(hipEventCreate(&b->evb0));
    HIP_TRY(hipEventCreate(&b->evb1));
    b->hist_first = std::max(1, env_int("YALPS_LPVAR_HIST", (int)HIST_FIRST)); // (test hook: forces the rerun)
    const int per_cu = env_int("YALPS_LPVAR_PER_CU", 0);                        // (test hook: one value for every class, a small grid)
    if (per_cu < 0 || per_cu > 8) return fail(YALPS_E_ARG, "YALPS_LPVAR_PER_CU: " + std::to_string(per_cu) + " is outside 1..8");
    for (int k = 0; k < NCLASS; k++) b->per_cu[k] = per_cu ? std::min(per_cu, kClasses[k].per_cu) : kClasses[k].per_cu;
    // (dynamic LDS beyond 48 KB: the attribute belongs to the function, raised once to the most a launch can ask for)
    for (const KernelForm &f : kForms)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(f.fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)SMALL_LDS_MAX));
    return 0;
}

int solve_impl(yalps_lpvar *b, int32_t w, int32_t h, int64_t ncells, const int32_t *brow, const int32_t *bcol, const double *bval,
               int32_t count, const int64_t *off, const int32_t *prow, const int32_t *pcol, const double *pval,
               const double *precision, const double *maxPivots, const int32_t *checkCycles, int32_t keep, int32_t *status_out,
               double *result_out, int64_t *pivots_out, float *gpu_ms_out) {
    if (int rc = validate(w, h, ncells, brow, bcol, count, off, prow, pcol)) return rc;
    if (ncells > 0 && !bval) return fail(YALPS_E_ARG, "yalps_lpvar_solve: base_val is NULL");
    if (count > 0 && (!precision || !maxPivots || !checkCycles || (off[count] > off[0] && !pval)))
        return fail(YALPS_E_ARG, "yalps_lpvar_solve: patch_val / precision / maxPivots / checkCycles is NULL");
    b->count = 0;
    b->keep = keep != 0;
    b->info = "launches=0 reruns=0\n";
    if (gpu_ms_out) *gpu_ms_out = 0.f;
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    const size_t n = (size_t)count, heven = ((size_t)h + 1) & ~(size_t)1, perm = (size_t)w + (size_t)h;
    const Shape S = shape_of(w, h);
    const int64_t base = off[0];
    const size_t npatch = (size_t)(off[count] - base);
    std::vector<VarDesc> D(n);
    for (size_t i = 0; i < n; i++) D[i] = VarDesc{off[i] - base, off[i + 1] - base, precision[i], maxPivots[i]};
    if (int rc = ensure(b->desc, sizeof(VarDesc) * n)) return rc;
    if (int rc = ensure(b->brow, sizeof(int32_t) * (size_t)ncells)) return rc;
    if (int rc = ensure(b->bcol, sizeof(int32_t) * (size_t)ncells)) return rc;
    if (int rc = ensure(b->bval, sizeof(double) * (size_t)ncells)) return rc;
    if (int rc = ensure(b->image, sizeof(double) * S.image_doubles)) return rc;
    if (int rc = ensure(b->prow, sizeof(int32_t) * npatch)) return rc;
    if (int rc = ensure(b->pcol, sizeof(int32_t) * npatch)) return rc;
    if (int rc = ensure(b->pval, sizeof(double) * npatch)) return rc;
    if (int rc = ensure(b->status, sizeof(int32_t) * n)) return rc;
    if (int rc = ensure(b->result, sizeof(double) * n)) return rc;
    if (int rc = ensure(b->pivots, sizeof(long long) * n)) return rc;
    if (int rc = ensure(b->col0, sizeof(double) * heven * n)) return rc;
    if (int rc = ensure(b->pos, sizeof(int32_t) * perm * n)) return rc;
    if (int rc = ensure(b->var, sizeof(int32_t) * perm * n)) return rc;
    if (b->keep)
        if (int rc = ensure(b->tab, sizeof(double) * (size_t)w * (size_t)h * n)) return rc;
    HIP_TRY(hipMemcpyAsync(b->desc.p, D.data(), sizeof(VarDesc) * n, hipMemcpyHostToDevice, s));
    if (ncells) {
        HIP_TRY(hipMemcpyAsync(b->brow.p, brow, sizeof(int32_t) * (size_t)ncells, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->bcol.p, bcol, sizeof(int32_t) * (size_t)ncells, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->bval.p, bval, sizeof(double) * (size_t)ncells, hipMemcpyHostToDevice, s));
    }
    if (npatch) {
        HIP_TRY(hipMemcpyAsync(b->prow.p, prow + base, sizeof(int32_t) * npatch, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->pcol.p, pcol + base, sizeof(int32_t) * npatch, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->pval.p, pval + base, sizeof(double) * npatch, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemsetAsync(b->status.p, 0x80, sizeof(int32_t) * n, s)); // (a status no kernel writes)
    b->h_status.assign(n, 0);
    b->w = w;
    b->h = h;
    b->count = count;

    // the image, once per call: zeros, then the base cells; the solving launches follow on the same stream
    float ms = 0.f;
    {
        const size_t units = S.image_doubles / 2;
        const int zgrid = (int)std::min<size_t>((units + 255) / 256, (size_t)b->num_cus * 8);
        const int sgrid = (int)std::min<size_t>(((size_t)ncells + 255) / 256, (size_t)b->num_cus * 8);
        double *image = static_cast<double *>(b->image.p);
        const int32_t *dr = static_cast<const int32_t *>(b->brow.p), *dc = static_cast<const int32_t *>(b->bcol.p);
        const double *dv = static_cast<const double *>(b->bval.p);
        HIP_TRY(hipEventRecord(b->evb0, s));
        lp_variants_base_kernel<<<dim3(std::max(1, zgrid)), dim3(256), 0, s>>>(image, (long long)S.image_doubles, dr, dc, dv,
                                                                                (long long)ncells, w, h, S.pitch, 0);
        HIP_TRY(hipGetLastError());
        if (ncells) {
            lp_variants_base_kernel<<<dim3(sgrid), dim3(256), 0, s>>>(image, (long long)S.image_doubles, dr, dc, dv, (long long)ncells,
                                                                      w, h, S.pitch, 1);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(b->evb1, s)); // (read after the first pass's wait: no wait of its own)
    }

    std::vector<int32_t> todo(n), rerun_all;
    for (size_t i = 0; i < n; i++) todo[i] = (int32_t)i;
    std::vector<Launch> launches;
    std::string text;
    long long hist_cap = b->hist_first;
    int nlaunches = 0, passes = 0;
    while (!todo.empty()) {
        if (int rc = run_pass(b, S, todo, checkCycles, hist_cap, launches, &ms)) return rc;
        if (passes == 0) {
            float image_ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&image_ms, b->evb0, b->evb1));
            ms += image_ms;
        }
        for (const Launch &L : launches) {
            char line[256];
            std::snprintf(line, sizeof line, "launch=%d pass=%d kernel=%s class=%d aux=%d lps=%zu grid=%d lds=%zu hist_cap=%lld\n", nlaunches++,
                          passes, form_name(*L.form).c_str(), S.cls, S.aux ? 1 : 0, L.vars.size(), L.grid, S.shmem, L.check ? hist_cap : 0ll);
            text += line;
        }
        // a variant whose phase outran the history left no output: grow the pool and rerun only those, from the image again
        std::vector<int32_t> again;
        for (int32_t i : todo) {
            if (b->h_status[i] == WG_HISTORY_FULL)
                again.push_back(i);
            else if (b->h_status[i] < 0 || b->h_status[i] > YALPS_CYCLED)
                return fail(YALPS_E_DEVICE, "lp_variants_kernel did not report a result for variant " + std::to_string(i));
        }
        rerun_all.insert(rerun_all.end(), again.begin(), again.end());
        todo.swap(again);
        hist_cap *= 4;
        passes++;
        if (!todo.empty() && hist_cap > (1ll << 28)) return fail(YALPS_E_NOMEM, "yalps_lpvar_solve: checkCycles history beyond 2^28 pivots");
    }
    std::string ids;
    for (int32_t i : rerun_all) ids += (ids.empty() ? "" : ",") + std::to_string(i);
    b->info = "launches=" + std::to_string(nlaunches) + " reruns=" + std::to_string(rerun_all.size()) + " rerun_lps=[" + ids + "]" +
              " base_cells=" + std::to_string((long long)ncells) + " patch_cells=" + std::to_string(npatch) +
              " image_bytes=" + std::to_string(sizeof(double) * S.image_doubles) + "\n" + text;

    b->h_col0.resize(heven * n);
    b->h_pos.resize(perm * n);
    b->h_var.resize(perm * n);
    HIP_TRY(hipMemcpyAsync(b->h_col0.data(), b->col0.p, sizeof(double) * heven * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->h_pos.data(), b->pos.p, sizeof(int32_t) * perm * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->h_var.data(), b->var.p, sizeof(int32_t) * perm * n, hipMemcpyDeviceToHost, s));
    if (result_out) HIP_TRY(hipMemcpyAsync(result_out, b->result.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (pivots_out) HIP_TRY(hipMemcpyAsync(pivots_out, b->pivots.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (status_out) std::memcpy(status_out, b->h_status.data(), sizeof(int32_t) * n);
    if (gpu_ms_out) *gpu_ms_out = ms;
    return 0;
}

void destroy_impl(yalps_lpvar *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (DevBuf *d : {&b->desc, &b->order, &b->counters, &b->brow, &b->bcol, &b->bval, &b->image, &b->prow, &b->pcol, &b->pval,
                      &b->status, &b->result, &b->pivots, &b->col0, &b->pos, &b->var, &b->tab, &b->ws, &b->hist})
        if (d->p) (void)hipFree(d->p);
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    if (b->evb0) (void)hipEventDestroy(b->evb0);
    if (b->evb1) (void)hipEventDestroy(b->evb1);
    if (b->own_stream && b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}
} // namespace

extern "C" {

const char *yalps_lpvar_last_error(void) { return g_err.c_str(); }

int32_t yalps_lpvar_validate(int32_t width, int32_t height, int64_t base_cells, const int32_t *base_row, const int32_t *base_col,
                             int32_t count, const int64_t *patch_offsets, const int32_t *patch_row, const int32_t *patch_col) {
    return validate(width, height, base_cells, base_row, base_col, count, patch_offsets, patch_row, patch_col);
}

int32_t yalps_lpvar_create(int32_t device, void *hip_stream, yalps_lpvar **out) {
    if (!out) return fail(YALPS_E_ARG, "yalps_lpvar_create: out is NULL");
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

void yalps_lpvar_destroy(yalps_lpvar *v) { destroy_impl(v); }

int32_t yalps_lpvar_solve(yalps_lpvar *v, int32_t width, int32_t height, int64_t base_cells, const int32_t *base_row,
                          const int32_t *base_col, const double *base_val, int32_t count, const int64_t *patch_offsets,
                          const int32_t *patch_row, const int32_t *patch_col, const double *patch_val, const double *precision,
                          const double *maxPivots, const int32_t *checkCycles, int32_t keep_tableaux, int32_t *status_out,
                          double *result_out, int64_t *pivots_out, float *gpu_ms_out) {
    if (!v) return fail(YALPS_E_ARG, "yalps_lpvar_solve: handle is NULL");
    const int32_t rc = solve_impl(v, width, height, base_cells, base_row, base_col, base_val, count, patch_offsets, patch_row,
                                  patch_col, patch_val, precision, maxPivots, checkCycles, keep_tableaux, status_out, result_out,
                                  pivots_out, gpu_ms_out);
    if (rc) v->count = 0; // (no last solve to read from)
    return rc;
}

int32_t yalps_lpvar_solution(yalps_lpvar *v, int32_t i, double *col0, int32_t *positionOfVariable, int32_t *variableAtPosition) {
    if (!v || i < 0 || i >= v->count) return fail(YALPS_E_ARG, "yalps_lpvar_solution: no such variant in the last solve");
    const size_t h = (size_t)v->h, heven = (h + 1) & ~(size_t)1, np = (size_t)v->w + h;
    if (col0) std::memcpy(col0, v->h_col0.data() + (size_t)i * heven, sizeof(double) * h);
    if (positionOfVariable) std::memcpy(positionOfVariable, v->h_pos.data() + (size_t)i * np, sizeof(int32_t) * np);
    if (variableAtPosition) std::memcpy(variableAtPosition, v->h_var.data() + (size_t)i * np, sizeof(int32_t) * np);
    return 0;
}

int32_t yalps_lpvar_tableau(yalps_lpvar *v, int32_t i, double *matrix) {
    if (!v || i < 0 || i >= v->count || !matrix) return fail(YALPS_E_ARG, "yalps_lpvar_tableau: no such variant in the last solve");
    if (!v->keep) return fail(YALPS_E_ARG, "yalps_lpvar_tableau: the last solve did not keep its tableaux (keep_tableaux)");
    const size_t wh = (size_t)v->w * (size_t)v->h;
    HIP_TRY(hipSetDevice(v->device));
    HIP_TRY(hipMemcpyAsync(matrix, static_cast<const double *>(v->tab.p) + (size_t)i * wh, sizeof(double) * wh, hipMemcpyDeviceToHost,
                           v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    return 0;
}

int32_t yalps_lpvar_info(const yalps_lpvar *v, char *buf, int32_t len) {
    if (!v || !buf || len < 1) return fail(YALPS_E_ARG, "yalps_lpvar_info: bad argument");
    const size_t n = std::min(v->info.size(), (size_t)len - 1);
    std::memcpy(buf, v->info.data(), n);
    buf[n] = 0;
    return (int32_t)std::min<size_t>(v->info.size(), INT32_MAX); // (the whole text's length: >= len means it was cut)
}

} // extern "C"
