// milp_dense_bounds_kernel.cuh -- milp_dense_kernel.cuh's two kernels for a call with variable bounds lb <= x <= ub: the root
// LPs with the bound rows between the equality rows and the binary rows and the shifted right-hand sides, and solution() moved
// back to x (both rules: dense_tableau.cuh, with the kind bytes).  Instantiated by milp_dense_bounds.hip alone
// (libyalps_milpdense_bounds.so).
#pragma once
#include "milp_dense_kernel.cuh"

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void milp_dense_bounds_root_kernel(MilpDenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, DenseJobBase<DenseTraits<true, false, true>>(L.call));
}

template <int T>
__global__ __launch_bounds__(T) void milp_dense_bounds_solution_kernel(MilpSolutionArgs a) {
    milp_dense_solution<T, DenseTraits<true, false, true>>(a);
}
