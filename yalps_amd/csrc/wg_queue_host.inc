// wg_queue_host.inc -- host side of the work-queue kernels (wg_queue.cuh): size classes, device buffers, the launches of a
// pass, the checkCycles history rerun.  Included inside the anonymous namespace of lp_batch.hip, lp_sens.hip, lp_variants.hip
// and milp_batch.hip after common.cuh, wg_simplex.cuh and the library's kernels: one text, four libraries.  Which kernels a
// pass launches is its caller's table (QUEUE_KERNEL_TABLE), so no library compiles a kernel of another through this text.
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
// Dynamic LDS is fixed per launch, so items are binned by what they need and every (class, checkCycles) pair is a launch
// of its own.  Classes 0..3 are the LDS form: an item of at most `lds_max` bytes, `per_cu` workgroups of `lanes` lanes per
// CU (160 KiB of LDS and 32 waves per CU: 8 x 19 KB x 4 waves, 4 x 39 KB, 2 x 79 KB, 1 x 150 KB x 16 waves); class 4 is
// the HBM form.  (profiles/lp_batch_classes.json holds the same-box table behind the lane counts.)
struct SizeClass {
    size_t lds_max;
    int lanes, per_cu;
};
constexpr int NCLASS = 5, HBM_CLASS = NCLASS - 1;
const SizeClass kClasses[NCLASS] = {{19 * 1024, 256, 8}, {39 * 1024, 256, 4}, {79 * 1024, 256, 2}, {SMALL_LDS_MAX, 1024, 1},
                                    {0, 1024, 1}};
constexpr long long QUEUE_MAX_BYTES = 4 << 20; // every library's YALPS_*_MAX_BYTES: the largest tableau a workgroup takes
constexpr size_t AUX_LDS_MAX = 64 * 1024; // HBM form: colbuf + prow stay in LDS up to this size, else behind the tableau in HBM
constexpr long long HIST_FIRST = 4096;    // first checkCycles history capacity per workgroup (YALPS_*_HIST)

int lp_class(int64_t w, int64_t h) {
    if (w < 1 || h < 1 || 8 * w * h > QUEUE_MAX_BYTES) return -1;
    const size_t bytes = small_lds_bytes((int)w, (int)h);
    for (int k = 0; k < HBM_CLASS; k++)
        if (bytes <= kClasses[k].lds_max) return k;
    return HBM_CLASS;
}
// HBM form: whether colbuf + prow of a w x h tableau go behind the tableau in the workspace (pcols + h > 8192)
bool lp_aux_hbm(int64_t w, int64_t h) { return sizeof(double) * ((size_t)small_pcols((int)w - 1) + (size_t)h) > AUX_LDS_MAX; }

// ---- a library's queue kernels: the six forms of one template, by name ---------------------------------------------
template <class LaunchT>
struct KernelForm {
    void (*fn)(LaunchT);
    int lanes;
    bool check, lds;
};
template <class LaunchT>
struct KernelTable {
    const char *name;
    KernelForm<LaunchT> forms[6];
};
#define QUEUE_KERNEL_TABLE(K)                                                                                                \
    {#K, {{K<256, false, true>, 256, false, true},     {K<256, true, true>, 256, true, true},                             \
          {K<1024, false, true>, 1024, false, true},   {K<1024, true, true>, 1024, true, true},                           \
          {K<1024, false, false>, 1024, false, false}, {K<1024, true, false>, 1024, true, false}}}

template <class LaunchT>
const KernelForm<LaunchT> *find_form(const KernelTable<LaunchT> &t, int lanes, bool check, bool lds) {
    for (const KernelForm<LaunchT> &f : t.forms)
        if (f.lanes == lanes && f.check == check && f.lds == lds) return &f;
    return nullptr;
}
template <class LaunchT>
std::string form_name(const KernelTable<LaunchT> &t, const KernelForm<LaunchT> &f) {
    return std::string(t.name) + "<" + std::to_string(f.lanes) + (f.check ? ",check" : "") + (f.lds ? ",lds" : "") + ">";
}
// (dynamic LDS beyond 48 KB: the attribute belongs to the function, raised once to the most a launch can ask for)
template <class LaunchT>
int raise_lds_limit(const KernelTable<LaunchT> &t) {
    for (const KernelForm<LaunchT> &f : t.forms)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(f.fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)SMALL_LDS_MAX));
    return 0;
}

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    template <class V>
    V *as() const { return static_cast<V *>(p); }
};

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
void release(std::initializer_list<DevBuf *> bufs) {
    for (DevBuf *d : bufs)
        if (d->p) (void)hipFree(d->p);
}

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

// cells [lo, hi) of row / col: inside the w x h tableau (1 <= w, h < 2^31) and strictly increasing by (row, col); 0, 1 = outside,
// 2 = order.  Every cell of a batch passes through this loop before it is uploaded.  With `x < 0 || x >= w` on the 64-bit bounds
// the compiler kept two compares per index, which the loop inside the LP validation had not had, and LpBatch.solve lost 6-8 %
// of its LPs per second on cell-heavy batches (profiles/queue_refactor_ab.json, "signed_cell_check"): hence the unsigned compares.
inline int check_cells(const int32_t *row, const int32_t *col, int64_t lo, int64_t hi, int64_t w, int64_t h, int64_t *at) {
    int64_t last = -1;
    for (int64_t c = lo; c < hi; c++) {
        if ((uint32_t)row[c] >= (uint64_t)h || (uint32_t)col[c] >= (uint64_t)w) return *at = c - lo, 1; // (one compare: negative is large)
        const int64_t key = (int64_t)row[c] * w + col[c];
        if (key <= last) return *at = c - lo, 2;
        last = key;
    }
    return 0;
}

// yalps_*_info: the text, cut to the caller's buffer
int32_t info_out(const std::string &info, char *buf, int32_t len) {
    const size_t n = std::min(info.size(), (size_t)len - 1);
    std::memcpy(buf, info.data(), n);
    buf[n] = 0;
    return (int32_t)std::min<size_t>(info.size(), INT32_MAX); // (the whole text's length: >= len means it was cut)
}

// ---- a handle's device: the card, the stream, the events around a pass, the class table as this process runs it -------
struct QueueDevice {
    int device = 0, num_cus = 256;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int lanes[NCLASS], per_cu[NCLASS];
};

int open_device(QueueDevice &q, int32_t device, void *hip_stream) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(YALPS_E_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(YALPS_E_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(YALPS_E_DEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only");
    q.device = device;
    q.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    for (int k = 0; k < NCLASS; k++) {
        q.lanes[k] = kClasses[k].lanes;
        q.per_cu[k] = kClasses[k].per_cu;
    }
    if (hip_stream) {
        q.stream = static_cast<hipStream_t>(hip_stream);
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&q.stream, hipStreamNonBlocking));
        q.own_stream = true;
    }
    HIP_TRY(hipEventCreate(&q.ev0));
    HIP_TRY(hipEventCreate(&q.ev1));
    return 0;
}
void close_device(QueueDevice &q) {
    if (q.ev0) (void)hipEventDestroy(q.ev0);
    if (q.ev1) (void)hipEventDestroy(q.ev1);
    if (q.own_stream && q.stream) (void)hipStreamDestroy(q.stream);
}

// ---- the buffers of a queue: what QueueLaunch points to ---------------------------------------------------------------
struct QueueBufs {
    DevBuf order, counters, ws, hist, status, result, pivots, col0, pos, var, tab;
    bool keep = false;
    long long hist_first = HIST_FIRST;
    std::vector<int32_t> h_status; // per item, after every pass
};
void release(QueueBufs &q) {
    release({&q.order, &q.counters, &q.ws, &q.hist, &q.status, &q.result, &q.pivots, &q.col0, &q.pos, &q.var, &q.tab});
}
// the outputs of n items
int ensure_outputs(QueueBufs &q, size_t n, size_t col0_total, size_t perm_total, size_t tab_total) {
    if (int rc = ensure(q.status, sizeof(int32_t) * n)) return rc;
    if (int rc = ensure(q.result, sizeof(double) * n)) return rc;
    if (int rc = ensure(q.pivots, sizeof(long long) * n)) return rc;
    if (int rc = ensure(q.col0, sizeof(double) * col0_total)) return rc;
    if (int rc = ensure(q.pos, sizeof(int32_t) * perm_total)) return rc;
    if (int rc = ensure(q.var, sizeof(int32_t) * perm_total)) return rc;
    if (q.keep)
        if (int rc = ensure(q.tab, sizeof(double) * tab_total)) return rc;
    return 0;
}
// after the inputs are on their way: every status set to one no kernel writes
int reset_status(QueueBufs &q, hipStream_t s, size_t n) {
    HIP_TRY(hipMemsetAsync(q.status.p, 0x80, sizeof(int32_t) * n, s));
    q.h_status.assign(n, 0);
    return 0;
}

struct Launch {
    int cls;
    bool check;
    std::vector<int32_t> items; // largest first
    int lanes, grid;
    size_t shmem;
    size_t stride; // HBM form: doubles of workspace per workgroup (tableau + colbuf / prow of its largest item)
    size_t at;     // where its items begin in the pass's order
};

// The launches of one pass over `todo`: binned by class x checkCycles, largest item first, grid, dynamic LDS and workspace
// stride of each; then the pass's buffers, its order uploaded and its counters zeroed.  shape(i, &w, &h) = checkCycles of i.
// (launches of one stream run one after the other: they share the workspace and the history pool)
template <class Shape>
int plan_launches(const QueueDevice &dev, QueueBufs &q, const std::vector<int32_t> &todo, Shape shape, long long hist_cap,
                  std::vector<Launch> &launches) {
    launches.clear();
    struct Bin {
        std::vector<std::pair<int64_t, int32_t>> items; // (area, item)
        size_t shmem = 0, stride = 0;
    } bins[2][NCLASS];
    // (the last shape's class and needs are kept, and an order that is already largest first is not sorted again: all variants
    // of a call share one shape, and without both LpVariants.solve lost 3-5 % on 4096 small variants, whose pass the variants
    // library used to plan with two compares per variant -- profiles/queue_refactor_ab.json, "planner_without_shape_cache")
    int lw = 0, lh = 0, lk = -1;
    size_t lshmem = 0, lstride = 0;
    for (int32_t i : todo) {
        int w = 0, h = 0;
        const bool check = shape(i, &w, &h);
        if (w != lw || h != lh) {
            lw = w, lh = h, lk = lp_class(w, h), lshmem = lstride = 0;
            if (lk >= 0 && lk != HBM_CLASS) {
                lshmem = small_lds_bytes(w, h);
            } else if (lk == HBM_CLASS) {
                const size_t lp = (size_t)small_pcols(w - 1), aux = lp + (size_t)h;
                if (!lp_aux_hbm(w, h)) lshmem = sizeof(double) * aux;
                lstride = (size_t)h * lp + ((aux + 1) & ~(size_t)1);
            }
        }
        if (lk < 0) continue;
        Bin &bin = bins[check][lk];
        bin.items.emplace_back((int64_t)w * h, i);
        bin.shmem = std::max(bin.shmem, lshmem);
        bin.stride = std::max(bin.stride, lstride);
    }
    size_t order_total = 0, ws_doubles = 0, hist_wgs = 0;
    for (int c = 0; c < 2; c++)
        for (int k = 0; k < NCLASS; k++) {
            Bin &bin = bins[c][k];
            if (bin.items.empty()) continue;
            const auto larger = [](const std::pair<int64_t, int32_t> &x, const std::pair<int64_t, int32_t> &y) { return x.first > y.first; };
            if (!std::is_sorted(bin.items.begin(), bin.items.end(), larger)) std::stable_sort(bin.items.begin(), bin.items.end(), larger);
            Launch L{k, c != 0, {}, 0, 0, 0, 0, 0};
            L.items.reserve(bin.items.size());
            for (const auto &e : bin.items) L.items.push_back(e.second);
            L.lanes = k != HBM_CLASS ? dev.lanes[k] : 1024;
            L.grid = (int)std::min<size_t>(L.items.size(), (size_t)dev.num_cus * (size_t)std::max(1, dev.per_cu[k]));
            L.shmem = std::max<size_t>((bin.shmem + 15) & ~(size_t)15, 16);
            L.stride = bin.stride;
            ws_doubles = std::max(ws_doubles, L.stride * (size_t)L.grid);
            if (L.check) hist_wgs = std::max(hist_wgs, (size_t)L.grid);
            L.at = order_total;
            order_total += L.items.size();
            launches.push_back(std::move(L));
        }
    if (launches.empty()) return 0;
    if (int rc = ensure(q.order, sizeof(int32_t) * order_total)) return rc;
    if (int rc = ensure(q.counters, sizeof(unsigned int) * launches.size())) return rc;
    if (int rc = ensure(q.ws, sizeof(double) * ws_doubles)) return rc;
    if (int rc = ensure(q.hist, sizeof(int32_t) * 2 * hist_wgs * (size_t)hist_cap)) return rc;
    std::vector<int32_t> order;
    order.reserve(order_total);
    for (const Launch &L : launches) order.insert(order.end(), L.items.begin(), L.items.end());
    HIP_TRY(hipMemcpyAsync(q.order.p, order.data(), sizeof(int32_t) * order_total, hipMemcpyHostToDevice, dev.stream));
    HIP_TRY(hipMemsetAsync(q.counters.p, 0, sizeof(unsigned int) * launches.size(), dev.stream));
    return 0;
}

// what a run of passes is called in messages and what it reports
struct QueueText {
    const char *lib;  // "yalps_lpbatch": no kernel of N lanes
    bool by_class;    // "yalps_lpvar": no kernel for class K
    const char *call; // "yalps_lpbatch_solve": checkCycles history beyond 2^28 pivots
    const char *item; // "LP": <kernel> did not report a result for LP i
};
struct QueueRun {
    int launches = 0, passes = 0;
    float ms = 0.f;
    std::vector<int32_t> reruns; // every item that ran again, in the order the passes met them
};

// Passes over items 0 .. n-1 until none is left with a full history.  One pass: every launch enqueued, then readback()
// (whatever the caller wants on its way back besides the statuses), one wait.  An item whose phase outran the history left no
// output but its status: the pool grows x 4 and only those run again, each from its own inputs, so a rerun starts clean.
// extra(a): the fields of LaunchT behind QueueLaunch.  line(L, kernel, pass, launch, hist_cap): one launch for the info text.
template <class LaunchT, class Shape, class Extra, class Readback, class Line>
int run_queue(const QueueDevice &dev, QueueBufs &q, const KernelTable<LaunchT> &table, const QueueText &txt, size_t n, Shape shape,
              Extra extra, Readback readback, Line line, QueueRun &run) {
    hipStream_t s = dev.stream;
    std::vector<int32_t> todo(n);
    for (size_t i = 0; i < n; i++) todo[i] = (int32_t)i;
    std::vector<Launch> launches;
    long long hist_cap = q.hist_first;
    while (!todo.empty()) {
        if (int rc = plan_launches(dev, q, todo, shape, hist_cap, launches)) return rc;
        for (const Launch &L : launches) // (before anything is enqueued)
            if (!find_form(table, L.lanes, L.check, L.cls != HBM_CLASS))
                return fail(YALPS_E_ARG, std::string(txt.lib) + (txt.by_class ? ": no kernel for class " + std::to_string(L.cls)
                                                                              : ": no kernel of " + std::to_string(L.lanes) + " lanes"));
        HIP_TRY(hipEventRecord(dev.ev0, s));
        for (size_t nl = 0; nl < launches.size(); nl++) {
            const Launch &L = launches[nl];
            const KernelForm<LaunchT> *form = find_form(table, L.lanes, L.check, L.cls != HBM_CLASS);
            LaunchT a{};
            a.order = q.order.as<const int32_t>() + L.at;
            a.count = (int32_t)L.items.size();
            a.counter = q.counters.as<unsigned int>() + nl;
            a.status = q.status.as<int32_t>();
            a.result = q.result.as<double>();
            a.pivots = q.pivots.as<long long>();
            a.col0 = q.col0.as<double>();
            a.pos = q.pos.as<int32_t>();
            a.var = q.var.as<int32_t>();
            a.tab = q.keep ? q.tab.as<double>() : nullptr;
            a.ws = q.ws.as<double>();
            a.ws_stride = (long long)L.stride;
            a.hist = q.hist.as<int32_t>();
            a.hist_cap = hist_cap;
            extra(a);
            form->fn<<<dim3(L.grid), dim3(form->lanes), L.shmem, s>>>(a);
            HIP_TRY(hipGetLastError());
            line(L, form_name(table, *form), run.passes, run.launches++, L.check ? hist_cap : 0ll);
        }
        HIP_TRY(hipEventRecord(dev.ev1, s));
        HIP_TRY(hipMemcpyAsync(q.h_status.data(), q.status.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
        if (int rc = readback()) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, dev.ev0, dev.ev1));
        run.ms += ms;
        std::vector<int32_t> again;
        for (int32_t i : todo) {
            if (q.h_status[i] == WG_HISTORY_FULL)
                again.push_back(i);
            else if (q.h_status[i] < 0 || q.h_status[i] > YALPS_CYCLED)
                return fail(YALPS_E_DEVICE, std::string(table.name) + " did not report a result for " + txt.item + " " + std::to_string(i));
        }
        run.reruns.insert(run.reruns.end(), again.begin(), again.end());
        todo.swap(again);
        hist_cap *= 4;
        run.passes++;
        if (!todo.empty() && hist_cap > (1ll << 28))
            return fail(YALPS_E_NOMEM, std::string(txt.call) + ": checkCycles history beyond 2^28 pivots");
    }
    return 0;
}

std::string join_ids(const std::vector<int32_t> &ids) {
    std::string out;
    for (int32_t i : ids) out += (out.empty() ? "" : ",") + std::to_string(i);
    return out;
}
