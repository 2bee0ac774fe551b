// lp_dense_free.hip -- libyalps_lpdense_free.so: the six lp_dense_free_kernel instantiations (lp_dense_kernel.cuh, the free traits)
// A code object of its own beside libyalps_lpdense.so and libyalps_lpdense_bounds.so: theirs hold the forms they held before free
// variables existed, and nothing else.  No host code but the table below; the C ABI, the pass and the handle are lp_dense.hip's,
// which launches these kernels through the pointers it gets here.
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
} // namespace

// The forms in QUEUE_KERNEL_TABLE's order: <256, false, true>, <256, true, true>, <1024, false, true>, <1024, true, true>,
// <1024, false, false>, <1024, true, false>.  Each is a void (*)(DenseLaunch).
extern "C" void yalps_lpdense_free_forms(void *out[6]) {
    out[0] = reinterpret_cast<void *>(lp_dense_free_kernel<256, false, true>);
    out[1] = reinterpret_cast<void *>(lp_dense_free_kernel<256, true, true>);
    out[2] = reinterpret_cast<void *>(lp_dense_free_kernel<1024, false, true>);
    out[3] = reinterpret_cast<void *>(lp_dense_free_kernel<1024, true, true>);
    out[4] = reinterpret_cast<void *>(lp_dense_free_kernel<1024, false, false>);
    out[5] = reinterpret_cast<void *>(lp_dense_free_kernel<1024, true, false>);
}
