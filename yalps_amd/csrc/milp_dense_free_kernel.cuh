// milp_dense_free_kernel.cuh -- milp_dense_bounds_kernel.cuh's two kernels for a call with free variables: the root LPs with one
// twin column per free variable behind the n originals, and solution() read off the wider tableau with the halves subtracted
// (both rules: dense_tableau.cuh).  lb and ub may both be absent.  milp_tree_kernel branches on the integer columns it is given:
// the host lists the twin of a free integer variable behind the n_int columns 1 + j, so that q is integral where p is.
// Instantiated by milp_dense_free.hip alone (libyalps_milpdense_free.so).
#pragma once
#include "milp_dense_bounds_kernel.cuh"

// The fill is inlined, unlike lp_dense_free_kernel's: this job has no `after`, so the <1024,check> HBM form keeps registers to
// spare, while as a call the fill itself spilled 36 bytes in all four 1024-lane forms -- a callee cannot borrow the registers
// its caller has free.
template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void milp_dense_free_root_kernel(MilpDenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, DenseJobBase<DenseTraits<true, true, true>>(L.call));
}

template <int T>
__global__ __launch_bounds__(T) void milp_dense_free_solution_kernel(MilpSolutionArgs a) {
    milp_dense_solution<T, DenseTraits<true, true, true>>(a);
}
