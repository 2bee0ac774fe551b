// milp_dense_free.hip -- libyalps_milpdense_free.so: the six milp_dense_free_root_kernel instantiations and
// milp_dense_free_solution_kernel (milp_dense_free_kernel.cuh).
// A code object of its own beside libyalps_milpdense.so and libyalps_milpdense_bounds.so: theirs hold the kernels they held
// before free variables existed, and nothing else.  No host code but the table below; the C ABI, the root pass, the tree pass
// and the handle are milp_dense.hip's, which launches these kernels through the pointers it gets here.
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
#include "milp_dense_free_kernel.cuh"
} // namespace

// The root forms in QUEUE_KERNEL_TABLE's order: <256, false, true>, <256, true, true>, <1024, false, true>,
// <1024, true, true>, <1024, false, false>, <1024, true, false>, each a void (*)(MilpDenseLaunch); then the epilogue <256>,
// a void (*)(MilpSolutionArgs).
extern "C" void yalps_milpdense_free_forms(void *out[7]) {
    out[0] = reinterpret_cast<void *>(milp_dense_free_root_kernel<256, false, true>);
    out[1] = reinterpret_cast<void *>(milp_dense_free_root_kernel<256, true, true>);
    out[2] = reinterpret_cast<void *>(milp_dense_free_root_kernel<1024, false, true>);
    out[3] = reinterpret_cast<void *>(milp_dense_free_root_kernel<1024, true, true>);
    out[4] = reinterpret_cast<void *>(milp_dense_free_root_kernel<1024, false, false>);
    out[5] = reinterpret_cast<void *>(milp_dense_free_root_kernel<1024, true, false>);
    out[6] = reinterpret_cast<void *>(milp_dense_free_solution_kernel<256>);
}
