// sim3.hip — Optimizer::OptimizeSim3 once the graph is built (reference src/orbslam/Optimizer.cc:1236-1449): the Sim3 alignment of
// LoopClosing::ComputeSim3, between Sim3Solver's RANSAC and the guided SearchBySim3 (LoopClosing.cc:300-350).
//
// One unknown, g2o::VertexSim3Expmap (unit quaternion, translation, scale; oplus(u) = Sim3(u) * estimate, u[6] = 0 under
// fix_scale), against two edges per correspondence with the map points held fixed:
//   EdgeSim3ProjectXYZ         e12 = obs1 - cam_map1(project(S12 . X2c))
//   EdgeInverseSim3ProjectXYZ  e21 = obs2 - cam_map2(project(S12^-1 . X1c))
// information invSigma2(octave) I2, a Huber kernel with delta = sqrt(th2) (float) on both, OptimizationAlgorithmLevenberg over a
// dense 7 x 7 system, and the reference's schedule: optimize(5), chi2 test of the PAIR (either edge > th2: both removed), fewer
// than 10 survivors -> return 0 with S12 unchanged, else optimize(10 if anything was removed, 5 if not), final chi2 test.
// The g2o arithmetic is restated in tests/sim3_restatement.py, which these kernels are checked against.
//
// The two edges have no analytic linearizeOplus: g2o differentiates them by BaseBinaryEdge's central differences, delta = 1e-9,
// through the vertex's oplus (push / oplus(+-delta e_d) / computeError / pop).  The 14 perturbed estimates Sim3(+-delta e_d) * S
// and their inverses do not depend on the edge: they are computed once per system build (threads 0..13) into LDS, and every edge
// maps its point through them — the same values g2o's per-edge push / oplus / pop gives.
//
// Like PoseOptimization (ba_solve.hip, pose_optimize_kernel), a latency chain of ~15 LM iterations x (build + trials) over
// <= ~2000 pairs: ONE launch of one persistent workgroup per problem (sivo_sim3_optimize_batch: k problems, k workgroups), every
// thread carrying the whole solver state and taking every decision itself from the same reduced sums.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "common.hpp"
#include "sim3_common.hpp"
#include "solver_common.hpp"
#include "solver_host.hpp"

#pragma clang fp contract(off)

namespace sivo {

// ------------------------------------------------------------------------------------------------
// the kernel
//
//   * the pairs (12 doubles: obs1, invSigma2_1, obs2, invSigma2_2, X1c, X2c) are read ONCE into LDS up to S3_CAP = 1536
//     (144 KB; the launch asks LDS for min(max n, S3_CAP) of them); pairs beyond that are read from memory in every pass;
//   * pair p is always handled by thread p % S3_THREADS: its flag byte (LDS, or the output array beyond the cap) needs no barrier;
//   * the 36 sums of a system build (28 of H, 7 of b, chi2) go through the halving butterfly over 64 slots, waves in index order
//     after that — one barrier per reduction (two alternating LDS buffers), a fixed summation order: bit-identical run to run;
//   * the system build has one more barrier: the 14 perturbed estimates and their inverses written to LDS by threads 0..13;
//   * the errors g2o keeps inside its edges are not stored: the chi2 tests read them at the estimate of the LAST TRIAL (accepted
//     or not — g2o does not recompute after a rejected step), 8 doubles every thread keeps;
//   * g2o solves the 7 x 7 system by a dense LDLT (LinearSolverDense, Eigen's pivoting LDLT); here a Cholesky with reciprocal
//     pivots, in natural order: the same solution up to rounding (1e-16 relative for the well-conditioned H + lambda I).
// ------------------------------------------------------------------------------------------------
constexpr int S3_THREADS = 256, S3_WAVES = S3_THREADS / 64, S3_CAP = 1536, S3_REC = 12;
constexpr size_t s3_lds_bytes(int cap) {
    return (size_t)cap * S3_REC * 8 + S3_CAP + 2 * S3_WAVES * 64 * 8 + 28 * 8 * 8;
}

struct Sim3Prob {              // one problem as staged on the device
    double s12[8], k1[4], k2[4];
    double delta, th2;         // Huber delta = (double)sqrtf(th2), th2 as double (the reference compares double chi2 > float th2)
    int64_t off;               // first pair in the pair array / the per-pair outputs
    int32_t n, fix_scale;
};
constexpr int S3_OUT = 12;     // per problem: s12[8], n_inliers, iterations, trials, (unused)

struct Sim3Args {
    const Sim3Prob *prob;
    const double *pairs;       // S3_REC doubles per pair, all problems back to back
    double *out;               // S3_OUT per problem
    double *chi2;              // 2 per pair: the chi2 of e12, e21 the last test read
    uint8_t *outlier;          // 1 per pair
    int lds_cap;               // pairs held in LDS (min(max n, S3_CAP))
};

struct Sim3Reducer {
    double *s_red;             // [2][S3_WAVES][64]
    int buf = 0;
    // v[0, 36) summed over the workgroup -> out[0, 36) in every thread.  After the butterfly, lane l holds slot bitreverse6(l).
    __device__ __forceinline__ void sum36(double (&v)[36], double (&out)[36]) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        double w[32];
        {   // first step on the 36 values (slots 36..63 are zero)
            const bool bit = lane & 1;
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const double hi = 32 + j < 36 ? v[32 + j < 36 ? 32 + j : 0] : 0.0;
                const double keep = bit ? hi : v[j], send = bit ? v[j] : hi;
                w[j] = keep + lane_xor<1>(send);
            }
        }
        halve_step<2, 16>(w, lane & 2);
        halve_step<4, 8>(w, lane & 4);
        halve_step<8, 4>(w, lane & 8);
        halve_step<16, 2>(w, lane & 16);
        halve_step<32, 1>(w, lane & 32);
        double *r = s_red + buf * (S3_WAVES * 64);
        r[wave * 64 + halving_slot<64>(lane)] = w[0];
        __syncthreads();
        double s = 0;
#pragma unroll
        for (int k = 0; k < S3_WAVES; ++k) s += r[k * 64 + lane];
        buf ^= 1;
#pragma unroll
        for (int k = 0; k < 36; ++k)
            out[k] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(s), k), __builtin_amdgcn_readlane(__double2loint(s), k));
    }
    __device__ __forceinline__ double sum1(double x) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        x += lane_xor<1>(x); x += lane_xor<2>(x); x += lane_xor<4>(x); x += lane_xor<8>(x); x += lane_xor<16>(x); x += lane_xor<32>(x);
        double *r = s_red + buf * (S3_WAVES * 64);
        if (lane == 0) r[wave] = x;
        __syncthreads();
        double s = 0;
#pragma unroll
        for (int k = 0; k < S3_WAVES; ++k) s += r[k];
        buf ^= 1;
        return s;
    }
};

struct S3Pair { double o1[2], is1, o2[2], is2, x1[3], x2[3]; };

// obs - cam_map(project(S . X)): (x / z) fx + cx
__device__ __forceinline__ void s3_err(const Sim3 &S, const double (&X)[3], const double (&obs)[2], const double (&K)[4], double (&e)[2]) {
    double Y[3];
    sim3_map(S, X, Y);
    e[0] = obs[0] - (Y[0] / Y[2] * K[0] + K[2]);
    e[1] = obs[1] - (Y[1] / Y[2] * K[1] + K[3]);
}
// e' (isig I) e as Eigen evaluates _error.dot(information() * _error)
__device__ __forceinline__ double s3_chi2(const double (&e)[2], double isig) { return e[0] * (isig * e[0]) + e[1] * (isig * e[1]); }

__global__ __launch_bounds__(S3_THREADS) void sim3_optimize_kernel(Sim3Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s3_lds[];
    const int cap = a.lds_cap;
    // (every region at a constant offset, the pair copy last: its size follows the launch)
    double *const s_red = reinterpret_cast<double *>(s3_lds);                  // [2][S3_WAVES][64]
    double *const sT = s_red + 2 * S3_WAVES * 64;                              // [28][8]: Sim3(+-delta e_d) * S, then the inverses
    uint8_t *const sF = reinterpret_cast<uint8_t *>(sT + 28 * 8);              // [S3_CAP]: outlier flag
    double *const sP = reinterpret_cast<double *>(sF + S3_CAP);                // [S3_REC][cap]
    const Sim3Prob &pr = a.prob[blockIdx.x];
    const int tid = threadIdx.x, n = pr.n;
    const int64_t off = pr.off;
    const double *const pairs = a.pairs + S3_REC * off;
    uint8_t *const gF = a.outlier + off;
    double *const gC = a.chi2 + 2 * off;
    double K1[4], K2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { K1[i] = pr.k1[i]; K2[i] = pr.k2[i]; }
    const double delta = pr.delta, th2 = pr.th2;
    const bool fix_scale = pr.fix_scale != 0;
    for (int p = tid; p < n && p < cap; p += S3_THREADS) {
        const double *q = pairs + S3_REC * (int64_t)p;
#pragma unroll
        for (int k = 0; k < S3_REC; ++k) sP[k * cap + p] = q[k];
        sF[p] = 0;
    }
    for (int p = cap + tid; p < n; p += S3_THREADS) gF[p] = 0;     // (pair p belongs to thread p % S3_THREADS: no barrier)
    // fn(p, pair, flag) over the pairs of this thread not flagged: the LDS copy first, then the pairs beyond it (two loops: one
    // load path each — a single loop whose load picks LDS or memory per pair turns the LDS pointer into a generic one)
    auto each_pair = [&](auto &&fn) {
        for (int p = tid; p < n && p < cap; p += S3_THREADS) {
            if (sF[p]) continue;
            S3Pair g;
            const double *q = sP + p;
            g.o1[0] = q[0]; g.o1[1] = q[cap]; g.is1 = q[2 * cap]; g.o2[0] = q[3 * cap]; g.o2[1] = q[4 * cap]; g.is2 = q[5 * cap];
            g.x1[0] = q[6 * cap]; g.x1[1] = q[7 * cap]; g.x1[2] = q[8 * cap]; g.x2[0] = q[9 * cap]; g.x2[1] = q[10 * cap]; g.x2[2] = q[11 * cap];
            fn(p, g, sF[p]);
        }
        for (int p = tid; p < n; p += S3_THREADS) {
            if (p < cap || gF[p]) continue;
            S3Pair g;
            const double *q = pairs + S3_REC * (int64_t)p;
            g.o1[0] = q[0]; g.o1[1] = q[1]; g.is1 = q[2]; g.o2[0] = q[3]; g.o2[1] = q[4]; g.is2 = q[5];
            g.x1[0] = q[6]; g.x1[1] = q[7]; g.x1[2] = q[8]; g.x2[0] = q[9]; g.x2[1] = q[10]; g.x2[2] = q[11];
            fn(p, g, gF[p]);
        }
    };
    auto load_T = [&](int k) {
        Sim3 S;
        const double *r = sT + 8 * k;
        S.q[0] = r[0]; S.q[1] = r[1]; S.q[2] = r[2]; S.q[3] = r[3]; S.t[0] = r[4]; S.t[1] = r[5]; S.t[2] = r[6]; S.s = r[7];
        return S;
    };
    Sim3Reducer red{s_red};

    Sim3 S, Seval;
#pragma unroll
    for (int i = 0; i < 4; ++i) S.q[i] = pr.s12[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) S.t[i] = pr.s12[4 + i];
    S.s = pr.s12[7];
    Seval = S;
    int iters = 0, trials = 0;

    // one g2o optimize(n_it) over the pairs not flagged (lambda re-initialised at its first iteration)
    auto optimize = [&](int n_it) {
        double H[28], b[7], lambda = 0, ni = 2, current = 0;
        for (int it = 0; it < n_it; ++it) {
            // the perturbed estimates of BaseBinaryEdge::linearizeOplus (oplus of +-delta e_d; u[6] = 0 under fix_scale)
            if (tid < 14) {
                double u[7] = {0, 0, 0, 0, 0, 0, 0};
                u[tid >> 1] = (tid & 1) ? -1e-9 : 1e-9;
                if (fix_scale) u[6] = 0;
                const Sim3 P = sim3_mul(sim3_exp(u), S), Pi = sim3_inv(P);
                double *r = sT + 8 * tid, *ri = sT + 8 * (14 + tid);
                r[0] = P.q[0]; r[1] = P.q[1]; r[2] = P.q[2]; r[3] = P.q[3]; r[4] = P.t[0]; r[5] = P.t[1]; r[6] = P.t[2]; r[7] = P.s;
                ri[0] = Pi.q[0]; ri[1] = Pi.q[1]; ri[2] = Pi.q[2]; ri[3] = Pi.q[3]; ri[4] = Pi.t[0]; ri[5] = Pi.t[1]; ri[6] = Pi.t[2]; ri[7] = Pi.s;
            }
            __syncthreads();
            const Sim3 Si = sim3_inv(S);
            // computeActiveErrors + buildSystem
            double acc[36];
#pragma unroll
            for (int k = 0; k < 36; ++k) acc[k] = 0.0;
            each_pair([&](int, const S3Pair &g, uint8_t &) {
#pragma unroll 1                                 // (not unrolled: the 14 perturbed maps of one side already fill the registers)
                for (int side = 0; side < 2; ++side) {
                    const double(&X)[3] = side == 0 ? g.x2 : g.x1;
                    const double(&obs)[2] = side == 0 ? g.o1 : g.o2;
                    const double(&K)[4] = side == 0 ? K1 : K2;
                    const double isig = side == 0 ? g.is1 : g.is2;
                    double e[2], J0[7], J1[7];
                    s3_err(side == 0 ? S : Si, X, obs, K, e);
#pragma unroll
                    for (int d = 0; d < 7; ++d) {
                        double ep[2], em[2];
                        s3_err(load_T(14 * side + 2 * d), X, obs, K, ep);
                        s3_err(load_T(14 * side + 2 * d + 1), X, obs, K, em);
                        J0[d] = (1.0 / (2 * 1e-9)) * (ep[0] - em[0]);
                        J1[d] = (1.0 / (2 * 1e-9)) * (ep[1] - em[1]);
                    }
                    const double c2 = s3_chi2(e, isig);
                    double r, w;
                    huber(c2, delta, r, w);
                    const double wo = w * isig;
                    int k = 0;
#pragma unroll
                    for (int i = 0; i < 7; ++i)
#pragma unroll
                        for (int j = i; j < 7; ++j) acc[k++] += wo * (J0[i] * J0[j] + J1[i] * J1[j]);
#pragma unroll
                    for (int i = 0; i < 7; ++i) acc[28 + i] -= wo * (J0[i] * e[0] + J1[i] * e[1]);
                    acc[35] += r;
                }
            });
            double Sm[36];
            red.sum36(acc, Sm);
#pragma unroll
            for (int i = 0; i < 28; ++i) H[i] = Sm[i];
#pragma unroll
            for (int i = 0; i < 7; ++i) b[i] = Sm[28 + i];
            current = Sm[35];
            if (it == 0) {                                   // computeLambdaInit: 1e-5 max |diag H|
                double md = 0;
                int k = 0;
#pragma unroll
                for (int i = 0; i < 7; ++i) { md = fmax(md, fabs(H[k])); k += 7 - i; }
                lambda = 1e-5 * md; ni = 2;
            }
            int qmax = 0;
            bool cont, term;
            do {
                double A[49], rd[7], x[7];
                {
                    int k = 0;
#pragma unroll
                    for (int i = 0; i < 7; ++i)
#pragma unroll
                        for (int j = i; j < 7; ++j) { A[7 * j + i] = H[k]; A[7 * i + j] = H[k]; ++k; }
                }
#pragma unroll
                for (int i = 0; i < 7; ++i) { A[8 * i] += lambda; x[i] = b[i]; }
                const Sim3 Sb = S;
                const bool ok = chol_recip<7>(A, rd);
                double scale = 0;
                if (ok) {
                    chol_recip_solve<7>(A, rd, x);
                    if (fix_scale) x[6] = 0;                     // oplusImpl writes the zero into the solver's x: computeScale sees it
                    S = sim3_mul(sim3_exp(x), Sb);
#pragma unroll
                    for (int i = 0; i < 7; ++i) scale += x[i] * (lambda * x[i] + b[i]);
                }
                Seval = S;
                const Sim3 Sti = sim3_inv(S);
                double chi = 0.0;
                each_pair([&](int, const S3Pair &g, uint8_t &) {
                    double e[2], r, w;
                    s3_err(S, g.x2, g.o1, K1, e);
                    huber(s3_chi2(e, g.is1), delta, r, w);
                    chi += r;
                    s3_err(Sti, g.x1, g.o2, K2, e);
                    huber(s3_chi2(e, g.is2), delta, r, w);
                    chi += r;
                });
                const double chi_sum = red.sum1(chi);
                const LmTrial tr = lm_trial(current, ok ? chi_sum : DBL_MAX, scale, lambda, ni);
                if (!tr.accepted) S = Sb;
                ++qmax; ++trials;
                cont = (tr.rho < 0 && qmax < 10);
                term = (qmax == 10 || tr.rho == 0);
            } while (cont);
            ++iters;
            if (term) break;
        }
    };
    // chi2 test over the pairs still in the graph, at the last trial's estimate; returns the number of pairs flagged
    auto chi2_test = [&]() {
        const Sim3 Sei = sim3_inv(Seval);
        double bad = 0.0;
        each_pair([&](int p, const S3Pair &g, uint8_t &flag) {
            double e[2];
            s3_err(Seval, g.x2, g.o1, K1, e);
            const double c12 = s3_chi2(e, g.is1);
            s3_err(Sei, g.x1, g.o2, K2, e);
            const double c21 = s3_chi2(e, g.is2);
            gC[2 * p] = c12; gC[2 * p + 1] = c21;
            if (c12 > th2 || c21 > th2) { flag = 1; bad += 1.0; }
        });
        return (int)red.sum1(bad);
    };

    int n_inliers = 0;
    const Sim3 S0 = S;
    if (n > 0) {
        optimize(5);
        const int n_bad = chi2_test();
        if (n - n_bad < 10) {
            S = S0;                                          // return 0: g2oS12 is not written back (:1420-1422)
        } else {
            optimize(n_bad > 0 ? 10 : 5);
            n_inliers = n - n_bad - chi2_test();
        }
    }
    for (int p = tid; p < n && p < cap; p += S3_THREADS) gF[p] = sF[p];
    if (tid == 0) {
        double *o = a.out + S3_OUT * (int64_t)blockIdx.x;
        o[0] = S.q[0]; o[1] = S.q[1]; o[2] = S.q[2]; o[3] = S.q[3]; o[4] = S.t[0]; o[5] = S.t[1]; o[6] = S.t[2]; o[7] = S.s;
        o[8] = n_inliers; o[9] = iters; o[10] = trials; o[11] = 0;
    }
}

static_assert(s3_lds_bytes(S3_CAP) <= 160 * 1024, "the LDS copy of the pairs must fit a CU");

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int sim3_run(SivoSim3Problem *probs, int k) {
    if (k < 0 || k > (1 << 20)) throw std::invalid_argument("problem count out of range");
    if (k > 0 && !probs) throw std::invalid_argument("null argument");
    int64_t total = 0;
    int max_n = 0;
    for (int i = 0; i < k; ++i) {
        const SivoSim3Problem &p = probs[i];
        if (p.n < 0 || p.n > (1 << 22)) throw std::invalid_argument("pair count out of range");
        if (p.n && !p.matches) throw std::invalid_argument("null argument");
        if (!(p.th2 >= 0.0f) || !std::isfinite(p.th2)) throw std::invalid_argument("th2 must be a finite non-negative number");
        if (!(p.s12[7] > 0.0) || !std::isfinite(p.s12[7])) throw std::invalid_argument("the Sim3 scale must be positive");
        total += p.n;
        max_n = std::max(max_n, p.n);
    }
    if (total > (int64_t)1 << 26) throw std::invalid_argument("pair count out of range");
    for (int i = 0; i < k; ++i) { probs[i].n_inliers = 0; probs[i].iterations = 0; probs[i].trials = 0; }
    if (k == 0) return SIVO_OK;
    require_device();
    // a loop closure evaluates its candidates on the loop-closing thread: one pinned buffer for the upload and the results, kept per thread
    static thread_local SolverCtx c(true, 256 << 10, 0, 256 << 10);
    c.bind();
    static int once[64];
    if (FirstUse first(once); first)
        SIVO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(sim3_optimize_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)s3_lds_bytes(S3_CAP)));
    // upload: the problem headers, then every problem's pairs back to back (staged in place); results: S3_OUT doubles per problem, 2 chi2
    // doubles and one flag byte per pair.  One copy each way, one launch, one synchronisation.
    Sim3Args a;
    Layout L;
    L.copy(a.prob, nullptr, sizeof(Sim3Prob) * (size_t)k);
    L.copy(a.pairs, nullptr, (size_t)total * sizeof(SivoSim3Match));
    L.take(a.out, (size_t)k * S3_OUT * 8); L.take(a.chi2, (size_t)total * 16); L.take(a.outlier, (size_t)total);
    L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
    Sim3Prob *hp = L.host(a.prob);
    unsigned char *hm = (unsigned char *)L.host(a.pairs);
    int64_t off = 0;
    for (int i = 0; i < k; ++i) {
        const SivoSim3Problem &p = probs[i];
        Sim3Prob &q = hp[i];
        std::memcpy(q.s12, p.s12, sizeof q.s12); std::memcpy(q.k1, p.k1, sizeof q.k1); std::memcpy(q.k2, p.k2, sizeof q.k2);
        q.delta = (double)std::sqrt(p.th2);                  // const float deltaHuber = sqrt(th2) (Optimizer.cc:1290): float sqrt
        q.th2 = (double)p.th2;
        q.off = off; q.n = p.n; q.fix_scale = p.fix_scale ? 1 : 0;
        if (p.n) std::memcpy(hm + (size_t)off * sizeof(SivoSim3Match), p.matches, (size_t)p.n * sizeof(SivoSim3Match));
        off += p.n;
    }
    a.lds_cap = std::max(1, std::min(max_n, S3_CAP));
    L.send(c.stream);
    hipLaunchKernelGGL(sim3_optimize_kernel, dim3(k), dim3(S3_THREADS), s3_lds_bytes(a.lds_cap), c.stream, a);
    SIVO_HIP(hipGetLastError());
    SIVO_HIP(hipMemcpyAsync(L.host(a.out), a.out, L.results(), hipMemcpyDeviceToHost, c.stream));
    SIVO_HIP(hipStreamSynchronize(c.stream));
    const double *res = L.host(a.out), *chi = L.host(a.chi2);
    const uint8_t *flag = L.host(a.outlier);
    for (int i = 0; i < k; ++i) {
        SivoSim3Problem &p = probs[i];
        const double *r = res + S3_OUT * (size_t)i;
        std::memcpy(p.s12, r, 64);
        p.n_inliers = (int)r[8]; p.iterations = (int)r[9]; p.trials = (int)r[10];
        const int64_t o = hp[i].off;
        for (int j = 0; j < p.n; ++j) {
            if (p.outlier) p.outlier[j] = flag[o + j];
            if (p.chi2_12) p.chi2_12[j] = chi[2 * (o + j)];
            if (p.chi2_21) p.chi2_21[j] = chi[2 * (o + j) + 1];
        }
    }
    return SIVO_OK;
}

}  // namespace sivo

using namespace sivo;

extern "C" int sivo_sim3_optimize(double s12[8], const double k1[4], const double k2[4], const SivoSim3Match *m, int n, float th2,
                                  int fix_scale, uint8_t *outlier, int *n_inliers, double *chi2_12, double *chi2_21, int *iterations,
                                  int *trials) {
    return guarded([&] {
        if (!s12 || !k1 || !k2 || !n_inliers) throw std::invalid_argument("null argument");
        SivoSim3Problem p;
        std::memset(&p, 0, sizeof p);
        std::memcpy(p.s12, s12, sizeof p.s12); std::memcpy(p.k1, k1, sizeof p.k1); std::memcpy(p.k2, k2, sizeof p.k2);
        p.matches = m; p.n = n; p.th2 = th2; p.fix_scale = fix_scale;
        p.outlier = outlier; p.chi2_12 = chi2_12; p.chi2_21 = chi2_21;
        *n_inliers = 0;
        if (iterations) *iterations = 0;
        if (trials) *trials = 0;
        const int rc = sim3_run(&p, 1);
        std::memcpy(s12, p.s12, sizeof p.s12);
        *n_inliers = p.n_inliers;
        if (iterations) *iterations = p.iterations;
        if (trials) *trials = p.trials;
        return rc;
    });
}

extern "C" int sivo_sim3_optimize_batch(SivoSim3Problem *problems, int n_problems) {
    return guarded([&] { return sim3_run(problems, n_problems); });
}
