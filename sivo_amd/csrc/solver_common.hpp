// solver_common.hpp — device pieces shared by the persistent-workgroup solvers (ba_solve.hip, sim3.hip): the Huber kernel of g2o's
// RobustKernelHuber and the fixed-order lane reductions.
#pragma once
#include <hip/hip_runtime.h>

namespace sivo {

__device__ __forceinline__ void huber(double c2, double delta, double &rho, double &w) {
    const double dsqr = delta * delta;
    if (c2 <= dsqr) { rho = c2; w = 1.0; }
    else { const double s = sqrt(c2); rho = 2 * s * delta - dsqr; w = delta / s; }
}

// x from lane (lane ^ M) for M = 1, 2, 8 on the VALU's data-parallel crossbar (no LDS traffic); 4, 16, 32 through ds_bpermute
template <int M>
__device__ __forceinline__ double lane_xor(double x) {
    static_assert(M == 1 || M == 2 || M == 4 || M == 8 || M == 16 || M == 32, "");
    if constexpr (M == 1 || M == 2 || M == 8) {
        constexpr int ctrl = M == 1 ? 0xB1 /* quad_perm [1,0,3,2] */ : M == 2 ? 0x4E /* quad_perm [2,3,0,1] */ : 0x128 /* row_ror:8 */;
        const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), ctrl, 0xf, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), ctrl, 0xf, 0xf, false);
        return __hiloint2double(hi, lo);
    } else {
        return __shfl_xor(x, M, 64);
    }
}

// One step of the halving butterfly: a lane whose bit M is clear keeps v[0, N) and hands v[N, 2N) to its partner, the other way
// round for a set bit; N values are left.
template <int M, int N>
__device__ __forceinline__ void halve_step(double *v, bool bit) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double keep = bit ? v[N + j] : v[j], send = bit ? v[j] : v[N + j];
        v[j] = keep + lane_xor<M>(send);
    }
}

template <int P>
__device__ __forceinline__ int halving_slot(int lane) {       // the slot whose total lane `lane` ends up with
    int s = 0;
#pragma unroll
    for (int b = 0; (1 << b) < P; ++b) s |= ((lane >> b) & 1) << ((P == 64 ? 5 : P == 32 ? 4 : 3) - b);
    return s;
}
}  // namespace sivo
