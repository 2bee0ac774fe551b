// lp_batch_host.inc -- host side of a batch of independent LPs: size classes, device buffers, the launches of a pass, the
// checkCycles history rerun.  Included by lp_batch.hip (libyalps_lpbatch.so) and by milp_batch.hip (libyalps_milpbatch.so, whose
// root pass is this code with kept tableaux) after common.cuh, wg_simplex.cuh and lp_batch_kernel.cuh: one text, two libraries.
// lp_sens.hip (libyalps_lpsens.so) includes it a third time around lp_sens_kernel: it sets the names below and LPB_SENS, which
// adds the buffer of the ranges; without them the text is what the two libraries above have always compiled.
#ifndef LPB_KERNEL
#define LPB_KERNEL lp_batch_kernel
#define LPB_KERNEL_NAME "lp_batch_kernel"
#define LPB_NAME "yalps_lpbatch"   // in messages
#define LPB_ENV "YALPS_LPBATCH"    // prefix of the environment switches
#endif
namespace {
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

// ---- size classes ------------------------------------------------------------------------------------------------
// Dynamic LDS is fixed per launch, so LPs are binned by what they need and every (class, checkCycles) pair is a launch
// of its own.  Classes 0..3 are the LDS form: an LP of at most `lds_max` bytes, `per_cu` workgroups of `lanes` lanes per
// CU (160 KiB of LDS and 32 waves per CU: 8 x 19 KB x 4 waves, 4 x 39 KB, 2 x 79 KB, 1 x 150 KB x 16 waves); class 4 is
// the HBM form.  (profiles/lp_batch_classes.json holds the same-box table behind the lane counts.)
struct SizeClass {
    size_t lds_max;
    int lanes, per_cu;
};
constexpr int NCLASS = YALPS_LPBATCH_CLASSES, HBM_CLASS = NCLASS - 1;
const SizeClass kClasses[NCLASS] = {{19 * 1024, 256, 8}, {39 * 1024, 256, 4}, {79 * 1024, 256, 2}, {SMALL_LDS_MAX, 1024, 1},
                                    {0, 1024, 1}};
constexpr size_t AUX_LDS_MAX = 64 * 1024; // HBM form: colbuf + prow stay in LDS up to this size, else behind the tableau in HBM
constexpr long long HIST_FIRST = 4096;    // first checkCycles history capacity per workgroup (YALPS_LPBATCH_HIST)

int lp_class(int64_t w, int64_t h) {
    if (w < 1 || h < 1 || 8 * w * h > YALPS_LPBATCH_MAX_BYTES) return -1;
    const size_t bytes = small_lds_bytes((int)w, (int)h);
    for (int k = 0; k < HBM_CLASS; k++)
        if (bytes <= kClasses[k].lds_max) return k;
    return HBM_CLASS;
}

using KernelFn = void (*)(LpLaunch);
struct KernelForm {
    KernelFn fn;
    int lanes;
    bool check, lds;
};
const KernelForm kForms[] = {
    {LPB_KERNEL<256, false, true>, 256, false, true},    {LPB_KERNEL<256, true, true>, 256, true, true},
    {LPB_KERNEL<1024, false, true>, 1024, false, true},  {LPB_KERNEL<1024, true, true>, 1024, true, true},
    {LPB_KERNEL<1024, false, false>, 1024, false, false}, {LPB_KERNEL<1024, true, false>, 1024, true, false},
};
// HBM form: whether colbuf + prow of a w x h tableau go behind the tableau in the workspace (pcols + h > 8192)
bool lp_aux_hbm(int64_t w, int64_t h) { return sizeof(double) * ((size_t)small_pcols((int)w - 1) + (size_t)h) > AUX_LDS_MAX; }

const KernelForm *find_form(int lanes, bool check, bool lds) {
    for (const KernelForm &f : kForms)
        if (f.lanes == lanes && f.check == check && f.lds == lds) return &f;
    return nullptr;
}
std::string form_name(const KernelForm &f) {
    return LPB_KERNEL_NAME "<" + std::to_string(f.lanes) + (f.check ? ",check" : "") + (f.lds ? ",lds" : "") + ">";
}

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

int env_int(const char *name, int dflt) {
    const char *v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}
// "a,b,c,..." over the classes, for same-box A/B runs of the class table (tools/lp_batch_throughput.py)
void env_list(const char *name, int *out, int n) {
    const char *v = std::getenv(name);
    for (int k = 0; v && *v && k < n; k++) {
        out[k] = std::atoi(v);
        v = std::strchr(v, ',');
        if (v) v++;
    }
}
} // namespace

struct yalps_lpbatch {
    int device = 0, num_cus = 256;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    long long hist_first = HIST_FIRST;
    int lanes[NCLASS], per_cu[NCLASS];
    DevBuf desc, order, counters, row, col, val, status, result, pivots, col0, pos, var, tab, ws, hist;
    // the last solve
    std::vector<LpDesc> descs;
    std::vector<double> h_col0;
    std::vector<int32_t> h_pos, h_var, h_status;
    bool keep = false;
    std::string info;
#ifdef LPB_SENS
    DevBuf sens;                 // per LP 3 * (w + h) doubles at 3 * perm_off: row0[w] col_up[w] col_dn[w] row_lo[h] row_hi[h]
    std::vector<double> h_sens;
#endif
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

int validate(int32_t count, const int32_t *width, const int32_t *height, const int64_t *off, const int32_t *row,
             const int32_t *col) {
    if (count < 0) return fail(YALPS_E_ARG, LPB_NAME ": count < 0");
    if (count == 0) return 0;
    if (!width || !height || !off) return fail(YALPS_E_ARG, LPB_NAME ": width / height / cell_offsets is NULL");
    if (off[0] < 0) return fail(YALPS_E_ARG, LPB_NAME ": LP 0: negative cell offset");
    for (int32_t i = 0; i < count; i++) {
        const std::string who = LPB_NAME ": LP " + std::to_string(i) + ": ";
        const int64_t w = width[i], h = height[i];
        if (w < 1 || h < 1) return fail(YALPS_E_ARG, who + "width and height must be at least 1");
        if (8 * w * h > YALPS_LPBATCH_MAX_BYTES)
            return fail(YALPS_E_ARG, who + "tableau of " + std::to_string(8 * w * h) + " bytes is above the batch limit of " +
                                         std::to_string((long long)YALPS_LPBATCH_MAX_BYTES));
        if (off[i + 1] < off[i]) return fail(YALPS_E_ARG, who + "cell offsets decrease");
        if (off[i + 1] > off[i] && (!row || !col)) return fail(YALPS_E_ARG, who + "row / col is NULL");
        int64_t last = -1;
        for (int64_t c = off[i]; c < off[i + 1]; c++) {
            if (row[c] < 0 || row[c] >= h || col[c] < 0 || col[c] >= w)
                return fail(YALPS_E_ARG, who + "cell " + std::to_string(c - off[i]) + " lies outside the tableau");
            const int64_t key = (int64_t)row[c] * w + col[c];
            if (key <= last) return fail(YALPS_E_ARG, who + "cells are not sorted by (row, col), strictly increasing");
            last = key;
        }
    }
    return 0;
}

struct Launch {
    int cls;
    bool check;
    std::vector<int32_t> lps; // largest first
    const KernelForm *form;
    int grid;
    size_t shmem;
    size_t stride; // HBM form: doubles of workspace per workgroup (tableau + colbuf / prow of its largest LP)
};

// One pass: the launches of `todo` (LP indices), all enqueued before one wait.  Leaves every LP's status in b->h_status.
int run_pass(yalps_lpbatch *b, const std::vector<int32_t> &todo, const int32_t *check, long long hist_cap,
             std::vector<Launch> &launches, float *ms_out) {
    hipStream_t s = b->stream;
    const std::vector<LpDesc> &D = b->descs;
    launches.clear();
    for (int c = 0; c < 2; c++)
        for (int k = 0; k < NCLASS; k++) {
            Launch L{k, c != 0, {}, nullptr, 0, 0, 0};
            for (int32_t i : todo)
                if ((check[i] != 0) == L.check && lp_class(D[i].w, D[i].h) == k) L.lps.push_back(i);
            if (L.lps.empty()) continue;
            std::stable_sort(L.lps.begin(), L.lps.end(), [&](int32_t x, int32_t y) {
                return (int64_t)D[x].w * D[x].h > (int64_t)D[y].w * D[y].h;
            });
            launches.push_back(std::move(L));
        }
    size_t order_total = 0, ws_doubles = 0, hist_wgs = 0;
    for (Launch &L : launches) {
        const bool lds = L.cls != HBM_CLASS;
        L.form = find_form(lds ? b->lanes[L.cls] : 1024, L.check, lds);
        if (!L.form) return fail(YALPS_E_ARG, LPB_NAME ": no kernel of " + std::to_string(b->lanes[L.cls]) + " lanes");
        L.grid = (int)std::min<size_t>(L.lps.size(), (size_t)b->num_cus * (size_t)std::max(1, b->per_cu[L.cls]));
        for (int32_t i : L.lps) {
            if (lds) {
                L.shmem = std::max(L.shmem, small_lds_bytes(D[i].w, D[i].h));
            } else {
                const size_t lp = (size_t)small_pcols(D[i].w - 1), aux = lp + (size_t)D[i].h;
                if (!D[i].aux_hbm) L.shmem = std::max(L.shmem, sizeof(double) * aux);
                L.stride = std::max(L.stride, (size_t)D[i].h * lp + ((aux + 1) & ~(size_t)1));
            }
        }
        L.shmem = std::max<size_t>((L.shmem + 15) & ~(size_t)15, 16);
        ws_doubles = std::max(ws_doubles, L.stride * (size_t)L.grid);
        if (L.check) hist_wgs = std::max(hist_wgs, (size_t)L.grid);
        order_total += L.lps.size();
    }
    if (launches.empty()) return 0;
    if (int rc = ensure(b->order, sizeof(int32_t) * order_total)) return rc;
    if (int rc = ensure(b->counters, sizeof(unsigned int) * launches.size())) return rc;
    if (int rc = ensure(b->ws, sizeof(double) * ws_doubles)) return rc;
    if (int rc = ensure(b->hist, sizeof(int32_t) * 2 * hist_wgs * (size_t)hist_cap)) return rc;
    std::vector<int32_t> order;
    order.reserve(order_total);
    for (const Launch &L : launches) order.insert(order.end(), L.lps.begin(), L.lps.end());
    HIP_TRY(hipMemcpyAsync(b->order.p, order.data(), sizeof(int32_t) * order_total, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(b->counters.p, 0, sizeof(unsigned int) * launches.size(), s));
    HIP_TRY(hipEventRecord(b->ev0, s));
    size_t at = 0, nl = 0;
    for (const Launch &L : launches) {
        LpLaunch a{};
        a.desc = static_cast<const LpDesc *>(b->desc.p);
        a.order = static_cast<const int32_t *>(b->order.p) + at;
        a.count = (int32_t)L.lps.size();
        a.counter = static_cast<unsigned int *>(b->counters.p) + nl;
        a.row = static_cast<const int32_t *>(b->row.p);
        a.col = static_cast<const int32_t *>(b->col.p);
        a.val = static_cast<const double *>(b->val.p);
        a.status = static_cast<int32_t *>(b->status.p);
        a.result = static_cast<double *>(b->result.p);
        a.pivots = static_cast<long long *>(b->pivots.p);
        a.col0 = static_cast<double *>(b->col0.p);
        a.pos = static_cast<int32_t *>(b->pos.p);
        a.var = static_cast<int32_t *>(b->var.p);
        a.tab = b->keep ? static_cast<double *>(b->tab.p) : nullptr;
        a.ws = static_cast<double *>(b->ws.p);
        a.ws_stride = (long long)L.stride;
        a.hist = static_cast<int32_t *>(b->hist.p);
        a.hist_cap = hist_cap;
#ifdef LPB_SENS
        a.sens = static_cast<double *>(b->sens.p);
#endif
        const KernelFn fn = L.form->fn;
        fn<<<dim3(L.grid), dim3(L.form->lanes), L.shmem, s>>>(a);
        HIP_TRY(hipGetLastError());
        at += L.lps.size();
        nl++;
    }
    HIP_TRY(hipEventRecord(b->ev1, s));
    HIP_TRY(hipMemcpyAsync(b->h_status.data(), b->status.p, sizeof(int32_t) * D.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    *ms_out += ms;
    return 0;
}

int create_impl(int32_t device, void *hip_stream, yalps_lpbatch **out) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(YALPS_E_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(YALPS_E_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(YALPS_E_DEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only");
    yalps_lpbatch *b = new yalps_lpbatch();
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
    b->hist_first = std::max(1, env_int(LPB_ENV "_HIST", (int)HIST_FIRST)); // (test hook: forces the rerun)
    for (int k = 0; k < NCLASS; k++) {
        b->lanes[k] = kClasses[k].lanes;
        b->per_cu[k] = kClasses[k].per_cu;
    }
    env_list(LPB_ENV "_LANES", b->lanes, HBM_CLASS);
    env_list(LPB_ENV "_PER_CU", b->per_cu, NCLASS);
    for (int k = 0; k < NCLASS; k++) {
        if (!find_form(b->lanes[k], false, k != HBM_CLASS))
            return fail(YALPS_E_ARG, LPB_ENV "_LANES: class " + std::to_string(k) + " has no kernel of " + std::to_string(b->lanes[k]) + " lanes (256 or 1024)");
        if (b->per_cu[k] < 1 || b->per_cu[k] > 8) // (32 waves per CU: at most eight workgroups of 256 lanes)
            return fail(YALPS_E_ARG, LPB_ENV "_PER_CU: class " + std::to_string(k) + ": " + std::to_string(b->per_cu[k]) + " is outside 1..8");
    }
    // (dynamic LDS beyond 48 KB: the attribute belongs to the function, raised once to the most a launch can ask for)
    for (const KernelForm &f : kForms)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(f.fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)SMALL_LDS_MAX));
    return 0;
}

int solve_impl(yalps_lpbatch *b, int32_t count, const int32_t *width, const int32_t *height, const int64_t *off,
               const int32_t *row, const int32_t *col, const double *val, const double *precision, const double *maxPivots,
               const int32_t *checkCycles, int32_t keep, int32_t *status_out, double *result_out, int64_t *pivots_out,
               float *gpu_ms_out) {
    if (int rc = validate(count, width, height, off, row, col)) return rc;
    if (count > 0 && (!precision || !maxPivots || !checkCycles || (off[count] > off[0] && !val)))
        return fail(YALPS_E_ARG, LPB_NAME "_solve: val / precision / maxPivots / checkCycles is NULL");
    b->descs.clear();
    b->keep = keep != 0;
    b->info = "launches=0 reruns=0\n";
    if (gpu_ms_out) *gpu_ms_out = 0.f;
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    const size_t n = (size_t)count;
    std::vector<LpDesc> &D = b->descs;
    D.resize(n);
    long long col0_total = 0, perm_total = 0, tab_total = 0;
    const int64_t base = off[0];
    for (size_t i = 0; i < n; i++) {
        LpDesc &d = D[i];
        d.w = width[i];
        d.h = height[i];
        d.cell_lo = off[i] - base;
        d.cell_hi = off[i + 1] - base;
        d.col0_off = col0_total;
        d.perm_off = perm_total;
        d.tab_off = tab_total;
        d.precision = precision[i];
        d.max_pivots = maxPivots[i];
        d.aux_hbm = lp_aux_hbm(d.w, d.h) ? 1 : 0;
        d.pad_ = 0;
        col0_total += (d.h + 1) & ~1; // (even offsets: 16-byte aligned column 0)
        perm_total += d.w + d.h;
        tab_total += (long long)d.w * d.h;
    }
    const size_t ncells = (size_t)(off[count] - base);
    if (int rc = ensure(b->desc, sizeof(LpDesc) * n)) return rc;
    if (int rc = ensure(b->row, sizeof(int32_t) * ncells)) return rc;
    if (int rc = ensure(b->col, sizeof(int32_t) * ncells)) return rc;
    if (int rc = ensure(b->val, sizeof(double) * ncells)) return rc;
    if (int rc = ensure(b->status, sizeof(int32_t) * n)) return rc;
    if (int rc = ensure(b->result, sizeof(double) * n)) return rc;
    if (int rc = ensure(b->pivots, sizeof(long long) * n)) return rc;
    if (int rc = ensure(b->col0, sizeof(double) * (size_t)col0_total)) return rc;
    if (int rc = ensure(b->pos, sizeof(int32_t) * (size_t)perm_total)) return rc;
    if (int rc = ensure(b->var, sizeof(int32_t) * (size_t)perm_total)) return rc;
    if (b->keep)
        if (int rc = ensure(b->tab, sizeof(double) * (size_t)tab_total)) return rc;
#ifdef LPB_SENS
    if (int rc = ensure(b->sens, sizeof(double) * 3 * (size_t)perm_total)) return rc;
#endif
    HIP_TRY(hipMemcpyAsync(b->desc.p, D.data(), sizeof(LpDesc) * n, hipMemcpyHostToDevice, s));
    if (ncells) {
        HIP_TRY(hipMemcpyAsync(b->row.p, row + base, sizeof(int32_t) * ncells, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->col.p, col + base, sizeof(int32_t) * ncells, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->val.p, val + base, sizeof(double) * ncells, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemsetAsync(b->status.p, 0x80, sizeof(int32_t) * n, s)); // (a status no kernel writes)
    b->h_status.assign(n, 0);

    std::vector<int32_t> todo(n), rerun_all;
    for (size_t i = 0; i < n; i++) todo[i] = (int32_t)i;
    std::vector<Launch> launches;
    std::string text;
    long long hist_cap = b->hist_first;
    int nlaunches = 0, passes = 0;
    float ms = 0.f;
    while (!todo.empty()) {
        if (int rc = run_pass(b, todo, checkCycles, hist_cap, launches, &ms)) return rc;
        for (const Launch &L : launches) {
            char line[256];
            std::snprintf(line, sizeof line, "launch=%d pass=%d kernel=%s class=%d lps=%zu grid=%d lds=%zu hist_cap=%lld\n", nlaunches++, passes,
                          form_name(*L.form).c_str(), L.cls, L.lps.size(), L.grid, L.shmem, L.check ? hist_cap : 0ll);
            text += line;
        }
        // an LP whose phase outran the history left no output: grow the pool and rerun only those (cells in, so a rerun starts clean)
        std::vector<int32_t> again;
        for (int32_t i : todo) {
            if (b->h_status[i] == WG_HISTORY_FULL)
                again.push_back(i);
            else if (b->h_status[i] < 0 || b->h_status[i] > YALPS_CYCLED)
                return fail(YALPS_E_DEVICE, LPB_KERNEL_NAME " did not report a result for LP " + std::to_string(i));
        }
        rerun_all.insert(rerun_all.end(), again.begin(), again.end());
        todo.swap(again);
        hist_cap *= 4;
        passes++;
        if (!todo.empty() && hist_cap > (1ll << 28)) return fail(YALPS_E_NOMEM, LPB_NAME "_solve: checkCycles history beyond 2^28 pivots");
    }
    std::string ids;
    for (int32_t i : rerun_all) ids += (ids.empty() ? "" : ",") + std::to_string(i);
    b->info = "launches=" + std::to_string(nlaunches) + " reruns=" + std::to_string(rerun_all.size()) + " rerun_lps=[" + ids + "]\n" + text;

    b->h_col0.resize((size_t)col0_total);
    b->h_pos.resize((size_t)perm_total);
    b->h_var.resize((size_t)perm_total);
    HIP_TRY(hipMemcpyAsync(b->h_col0.data(), b->col0.p, sizeof(double) * (size_t)col0_total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->h_pos.data(), b->pos.p, sizeof(int32_t) * (size_t)perm_total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->h_var.data(), b->var.p, sizeof(int32_t) * (size_t)perm_total, hipMemcpyDeviceToHost, s));
#ifdef LPB_SENS
    b->h_sens.resize(3 * (size_t)perm_total);
    HIP_TRY(hipMemcpyAsync(b->h_sens.data(), b->sens.p, sizeof(double) * 3 * (size_t)perm_total, hipMemcpyDeviceToHost, s));
#endif
    if (result_out) HIP_TRY(hipMemcpyAsync(result_out, b->result.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (pivots_out) HIP_TRY(hipMemcpyAsync(pivots_out, b->pivots.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (status_out) std::memcpy(status_out, b->h_status.data(), sizeof(int32_t) * n);
    if (gpu_ms_out) *gpu_ms_out = ms;
    return 0;
}

void lpbatch_destroy_impl(yalps_lpbatch *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (DevBuf *d : {&b->desc, &b->order, &b->counters, &b->row, &b->col, &b->val, &b->status, &b->result, &b->pivots, &b->col0,
                      &b->pos, &b->var, &b->tab, &b->ws, &b->hist})
        if (d->p) (void)hipFree(d->p);
#ifdef LPB_SENS
    if (b->sens.p) (void)hipFree(b->sens.p);
#endif
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    if (b->own_stream && b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

// create_impl, with a half-made handle taken down again and the reason kept
int lpbatch_create(int32_t device, void *hip_stream, yalps_lpbatch **out) {
    *out = nullptr;
    const int rc = create_impl(device, hip_stream, out);
    if (rc && *out) {
        const std::string why = g_err;
        lpbatch_destroy_impl(*out);
        *out = nullptr;
        g_err = why;
    }
    return rc;
}
} // namespace
