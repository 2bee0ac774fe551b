// lp_batch_lib.inc -- how libyalps_lpbatch.so names itself to lp_batch_host.inc, and its handle.  Included at file scope by
// lp_batch.hip and by milp_batch.hip, whose root pass keeps that library's kernels, names and switches.
namespace {
static_assert(YALPS_LPBATCH_MAX_BYTES == QUEUE_MAX_BYTES && YALPS_LPBATCH_CLASSES == NCLASS, "include/yalps_lpbatch.h");
const KernelTable<LpLaunch> kLpKernels = QUEUE_KERNEL_TABLE(lp_batch_kernel);
struct LpBatchLib {
    using Launch = LpLaunch;
    static constexpr const char *name = "yalps_lpbatch", *env = "YALPS_LPBATCH";
    static constexpr bool sens = false;
    static const KernelTable<LpLaunch> &kernels() { return kLpKernels; }
};
} // namespace

struct yalps_lpbatch : LpPass<LpBatchLib> {};
