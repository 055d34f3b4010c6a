// solver_common.hpp — device pieces shared by the persistent-workgroup solvers (ba_solve.hip, sim3.hip, essential_graph.hip): the Huber
// kernel of g2o's RobustKernelHuber, the fixed-order lane reductions and a small dense Cholesky.
#pragma once
#include <hip/hip_runtime.h>

namespace sivo {

__device__ __forceinline__ void huber(double c2, double delta, double &rho, double &w) {
    const double dsqr = delta * delta;
    if (c2 <= dsqr) { rho = c2; w = 1.0; }
    else { const double s = sqrt(c2); rho = 2 * s * delta - dsqr; w = delta / s; }
}

// g2o's OptimizationAlgorithmLevenberg::solve after one trial of chi2 `temp` (DBL_MAX when the system could not be solved): rho from the
// chi2 `current` of the linearisation point and computeScale's `scale`; an accepted trial (rho > 0, temp finite) becomes `current` and
// shrinks lambda, a rejected one grows lambda by ni and doubles ni.  The cube is t * t * t where g2o calls pow(t, 3), in every solver.
struct LmTrial { double rho; bool accepted; };
__device__ __forceinline__ LmTrial lm_trial(double &current, double temp, double scale, double &lambda, double &ni) {
    const double rho = (current - temp) / (scale + 1e-3);
    const bool accepted = rho > 0 && isfinite(temp);
    if (accepted) {
        const double t = 2 * rho - 1;
        double alpha = 1. - t * t * t;
        alpha = fmin(alpha, 2. / 3.);
        lambda *= fmax(1. / 3., alpha);
        ni = 2; current = temp;
    } else {
        lambda *= ni; ni *= 2;
    }
    return {rho, accepted};
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

// lower Cholesky factor of the N x N matrix A (row-major, lower triangle read), the reciprocals of its diagonal in rd
template <int N>
__device__ __forceinline__ bool chol_recip(double (&A)[N * N], double (&rd)[N]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = A[j * N + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= A[j * N + k] * A[j * N + k];
        ok = ok && (d > 0.0);
        d = sqrt(d);
        A[j * N + j] = d;
        rd[j] = 1.0 / d;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double s = A[i * N + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= A[i * N + k] * A[j * N + k];
            A[i * N + j] = s * rd[j];
        }
    }
    return ok;
}
template <int N>
__device__ __forceinline__ void chol_recip_solve(const double (&L)[N * N], const double (&rd)[N], double (&x)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i * N + k] * x[k];
        x[i] = s * rd[i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) s -= L[k * N + i] * x[k];
        x[i] = s * rd[i];
    }
}
}  // namespace sivo
