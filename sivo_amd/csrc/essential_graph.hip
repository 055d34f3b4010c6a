// essential_graph.hip — Optimizer::OptimizeEssentialGraph once the graph is built (reference src/orbslam/Optimizer.cc:928-1233): the
// Sim3 pose graph LoopClosing::CorrectLoop optimises after a loop closure (LoopClosing.cc:582), and the map-point correction behind it.
//
// One g2o::VertexSim3Expmap per keyframe (oplus(u) = Sim3(u) * estimate, u[6] = 0 under fix_scale), EdgeSim3 edges with information
// I7 and no robust kernel:  e = log(Sji * Si * Sj^-1)  (g2o's Sim3::log).  EdgeSim3 has no analytic linearizeOplus: BaseBinaryEdge
// differentiates it by central differences, delta = 1e-9, through each free vertex's oplus.  The 14 perturbed estimates of a vertex
// (Sim3(+-delta e_d) * S, and their inverses for the vertex-1 side) do not depend on the edge: they are formed once per vertex per
// build.  OptimizationAlgorithmLevenberg with setUserLambdaInit(1e-16), optimize(20), g2o's accept / reject rule, 10 trials at most.
// The arithmetic is restated in tests/essential_graph_restatement.py, which these kernels are checked against.
//
// The linear system is sparse: 7 x 7 blocks, one block row per free vertex on an edge.  The host orders the variables (minimum degree
// on the block graph, ties to the lower vertex index) and factors the pattern symbolically ONCE per call: the blocks of L, the
// elimination tree, its levels, and for every block of L the list of (L_ik, L_jk) products its left-looking update sums.  The
// device does the numeric work: per trial, H + lambda I is factored by block Cholesky level by level (every column of a level is
// independent), then the two triangular solves walk the levels up and down.  No floating-point atomics anywhere: every sum has one
// owner and a host-fixed order, so results are bit-identical run to run.
//
// LM state in device memory (EgLm), as ba_solve.hip does it: the host enqueues STEPS — [linearise if due: perturbed
// estimates, 29 errors per edge, H / b blocks] -> factor + solve (one workgroup) -> trial estimates -> trial errors and chi2, whose
// last workgroup takes the decision — and reads the state once per batch.  A step after `done` is six empty launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "common.hpp"
#include "sim3_common.hpp"
#include "solver_common.hpp"
#include "solver_host.hpp"
#include "sparse_plan.hpp"

#pragma clang fp contract(off)

namespace sivo {

// ------------------------------------------------------------------------------------------------
// g2o::Sim3::log (types/sim3/sim3.h), branch by branch: |sigma| < 1e-5 or not, d = (tr R - 1) / 2 > 1 - 1e-5 or not
// ------------------------------------------------------------------------------------------------
// Eigen's Quaternion::toRotationMatrix
__device__ __forceinline__ void quat_to_rot(const double (&q)[4], double (&R)[9]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                 tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// W.lu().solve(t) for the 3 x 3 W: partial pivoting (first largest |entry| of the column), unit lower L, then U
__device__ __forceinline__ void lu3_solve(double (&M)[9], double (&b)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int p = k;
        double amax = fabs(M[4 * k]);
#pragma unroll
        for (int i = k + 1; i < 3; ++i)
            if (fabs(M[3 * i + k]) > amax) { amax = fabs(M[3 * i + k]); p = i; }
        if (p != k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { const double t = M[3 * k + c]; M[3 * k + c] = M[3 * p + c]; M[3 * p + c] = t; }
            const double t = b[k]; b[k] = b[p]; b[p] = t;
        }
        if (M[4 * k] != 0.0) {
#pragma unroll
            for (int i = k + 1; i < 3; ++i) M[3 * i + k] = M[3 * i + k] / M[4 * k];
        }
#pragma unroll
        for (int i = k + 1; i < 3; ++i)
#pragma unroll
            for (int c = k + 1; c < 3; ++c) M[3 * i + c] = M[3 * i + c] - M[3 * i + k] * M[3 * k + c];
    }
#pragma unroll
    for (int i = 1; i < 3; ++i)
#pragma unroll
        for (int m = 0; m < i; ++m) b[i] = b[i] - M[3 * i + m] * b[m];
#pragma unroll
    for (int i = 2; i >= 0; --i) {
#pragma unroll
        for (int m = i + 1; m < 3; ++m) b[i] = b[i] - M[3 * i + m] * b[m];
        b[i] = b[i] / M[4 * i];
    }
}

__device__ __forceinline__ void sim3_log(const Sim3 &S, double (&res)[7]) {
    const double s = S.s;
    const double sigma = log(s);
    double R[9];
    quat_to_rot(S.q, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double eps = 0.00001;
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};          // deltaR(R)
    const bool near = d > 1 - eps;
    double theta = 0.0, f = 0.5;
    if (!near) {
        theta = acos(d);
        f = theta / (2 * sqrt(1 - d * d));
    }
    const double om[3] = {f * dR[0], f * dR[1], f * dR[2]};
    double A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (near) {
            A = 1. / 2.; B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        const double sigma2 = sigma * sigma;
        if (near) {
            A = ((sigma - 1) * s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta2 = theta * theta;
            const double a = s * sin(theta), b = s * cos(theta), c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    const double Om[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double W[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double o2 = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
            W[3 * i + j] = A * Om[3 * i + j] + B * o2 + C * (i == j ? 1.0 : 0.0);
        }
    double ups[3] = {S.t[0], S.t[1], S.t[2]};
    lu3_solve(W, ups);
    res[0] = om[0]; res[1] = om[1]; res[2] = om[2]; res[3] = ups[0]; res[4] = ups[1]; res[5] = ups[2]; res[6] = sigma;
}

// EdgeSim3::computeError: log(C * Si * Sj^-1)
__device__ __forceinline__ void eg_error(const Sim3 &C, const Sim3 &Si, const Sim3 &Sj_inv, double (&e)[7]) {
    sim3_log(sim3_mul(sim3_mul(C, Si), Sj_inv), e);
}

__device__ __forceinline__ Sim3 load_sim3(const double *p) {
    Sim3 S;
    S.q[0] = p[0]; S.q[1] = p[1]; S.q[2] = p[2]; S.q[3] = p[3]; S.t[0] = p[4]; S.t[1] = p[5]; S.t[2] = p[6]; S.s = p[7];
    return S;
}
__device__ __forceinline__ void store_sim3(double *p, const Sim3 &S) {
    p[0] = S.q[0]; p[1] = S.q[1]; p[2] = S.q[2]; p[3] = S.q[3]; p[4] = S.t[0]; p[5] = S.t[1]; p[6] = S.t[2]; p[7] = S.s;
}

// ------------------------------------------------------------------------------------------------
// device state and arguments
// ------------------------------------------------------------------------------------------------
constexpr int EG_T = 256, EG_GRID = 8;      // the multi-workgroup kernels: EG_GRID workgroups of EG_T threads, grid-stride
constexpr int EG_FT = 1024;                 // the factor / solve kernel: ONE workgroup of 16 waves
constexpr int EG_NERR = 29;                 // errors per edge and build: at the estimate, 14 perturbations of vertex 0, 14 of vertex 1

// g2o::SparseOptimizer::optimize / OptimizationAlgorithmLevenberg::solve as device state (the host loop of ba_solve.hip's BaLm)
struct EgLm {
    double lambda, ni, current, rho, chi_init, scale;
    int cur;                    // est[cur]: the current estimate, est[cur ^ 1]: the trial
    int need_lin;               // the next step starts an iteration (linearisation)
    int it, it_limit, qmax, done, trials, ok;
};

struct EgDev {
    double *est0, *est1;        // 8 per vertex (all n vertices)
    const int *vpos;            // vertex -> elimination position of its variable, -1: fixed or without edges
    const int *eij;             // 2 per edge
    const double *meas;         // 8 per edge
    double *pert;               // 28 x 8 per position: Sim3(+-delta e_d) * S (14), then the inverses (14)
    double *errs;               // EG_NERR x 7 per edge
    double *chi;                // per edge, the trial's e'e
    const int *own_blk, *own_ptr, *own_con;    // assembly owners: L block, contribution range; contribution = edge * 4 + rowside * 2 + colside
    double *H;                  // 49 per L block (the fill blocks stay zero)
    double *b;                  // 7 per position
    double *L;                  // 49 per L block (diagonal blocks first: block p = position p)
    double *rinv;               // 7 per position: 1 / L_pp[r][r]
    double *x;                  // 7 per position: the forward solve's y, then the solution
    const int *lvl_ptr, *lvl_col;              // levels of the elimination tree: positions per level
    const int *off_ptr, *off_blk;              // the off-diagonal L blocks of each level's columns
    const int *blk_col;         // per L block: its column (diagonal blocks: the position)
    const int *pair_ptr, *pairs;               // per L block: the (L_ik, L_jk) block pairs its update sums (diagonal: L_jk twice)
    const int *row_ptr, *row_lst;              // per position j: the blocks (j, k < j) of L, with k: 2 ints each
    const int *col_ptr, *col_lst;              // per position j: the blocks (i > j, j) of L, with i: 2 ints each
    EgLm *lm;
    unsigned *counter;
    int n, ne, na, nlev, n_own, fix_scale;
};

__device__ __forceinline__ double *eg_est(const EgDev &d, int k) { return k ? d.est1 : d.est0; }

// ------------------------------------------------------------------------------------------------
// linearisation (the first step of an iteration)
// ------------------------------------------------------------------------------------------------
// the 14 perturbed estimates of every free vertex and their inverses (BaseBinaryEdge::linearizeOplus: push / oplus(+-delta e_d) / pop)
__global__ __launch_bounds__(EG_T) void eg_perturb_kernel(EgDev d) {
    if (d.lm->done || !d.lm->need_lin) return;
    const double *est = eg_est(d, d.lm->cur);
    for (int t = blockIdx.x * EG_T + threadIdx.x; t < d.n * 14; t += EG_GRID * EG_T) {
        const int v = t / 14, k = t % 14, p = d.vpos[v];
        if (p < 0) continue;
        double u[7] = {0, 0, 0, 0, 0, 0, 0};
        u[k >> 1] = (k & 1) ? -1e-9 : 1e-9;
        if (d.fix_scale) u[6] = 0;
        const Sim3 P = sim3_mul(sim3_exp(u), load_sim3(est + 8 * (int64_t)v));
        store_sim3(d.pert + (int64_t)p * 224 + 8 * k, P);
        store_sim3(d.pert + (int64_t)p * 224 + 8 * (14 + k), sim3_inv(P));
    }
}

// the 29 errors of every edge at the current estimate: k = 0 unperturbed, 1..14 vertex 0 perturbed, 15..28 vertex 1 perturbed
__global__ __launch_bounds__(EG_T) void eg_errors_kernel(EgDev d) {
    if (d.lm->done || !d.lm->need_lin) return;
    const double *est = eg_est(d, d.lm->cur);
    const int64_t total = (int64_t)d.ne * EG_NERR;
    for (int64_t t = blockIdx.x * EG_T + threadIdx.x; t < total; t += EG_GRID * EG_T) {
        const int e = (int)(t / EG_NERR), k = (int)(t % EG_NERR);
        const int vi = d.eij[2 * e], vj = d.eij[2 * e + 1];
        const int pi = d.vpos[vi], pj = d.vpos[vj];
        if ((k >= 1 && k <= 14 && pi < 0) || (k >= 15 && pj < 0)) continue;          // (a fixed side has no Jacobian)
        const Sim3 C = load_sim3(d.meas + 8 * (int64_t)e);
        Sim3 Si, Sji;
        if (k >= 1 && k <= 14) Si = load_sim3(d.pert + (int64_t)pi * 224 + 8 * (k - 1));
        else Si = load_sim3(est + 8 * (int64_t)vi);
        if (k >= 15) Sji = load_sim3(d.pert + (int64_t)pj * 224 + 8 * (14 + k - 15));
        else Sji = sim3_inv(load_sim3(est + 8 * (int64_t)vj));
        double er[7];
        eg_error(C, Si, Sji, er);
        double *o = d.errs + t * 7;
#pragma unroll
        for (int m = 0; m < 7; ++m) o[m] = er[m];
    }
}

// H and b, block by block: ONE wave per owner block of L (diagonal blocks and the off-diagonal blocks an edge touches), lane
// r * 7 + c of entry (r, c), lanes 49..55 of b (diagonal owners).  The owner sums its contributions in the host's order: per edge
// J_row^T J_col (the side of the block's row, the side of its column), each entry a sum over the 7 error components in order.
__global__ __launch_bounds__(EG_T) void eg_assemble_kernel(EgDev d) {
    if (d.lm->done || !d.lm->need_lin) return;
    const int lane = threadIdx.x & 63;
    const int r = lane / 7, c = lane % 7;
    constexpr double scalar = 1.0 / (2 * 1e-9);
    for (int o = blockIdx.x * (EG_T / 64) + (threadIdx.x >> 6); o < d.n_own; o += EG_GRID * (EG_T / 64)) {
        const int blk = d.own_blk[o];
        double acc = 0.0;
        for (int q = d.own_ptr[o]; q < d.own_ptr[o + 1]; ++q) {
            const int con = d.own_con[q], e = con >> 2, rs = (con >> 1) & 1, cs = con & 1;
            const double *E = d.errs + (int64_t)e * EG_NERR * 7;
            if (lane < 49) {
                // J_side[m][dof] = (e(+delta e_dof) - e(-delta e_dof))[m] / (2 delta)
                const double *Pr = E + 7 * (1 + 14 * rs + 2 * r), *Pc = E + 7 * (1 + 14 * cs + 2 * c);
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < 7; ++m) s += (scalar * (Pr[m] - Pr[7 + m])) * (scalar * (Pc[m] - Pc[7 + m]));
                acc += s;
            } else if (lane < 56) {
                const int rr = lane - 49;
                const double *Pr = E + 7 * (1 + 14 * rs + 2 * rr);
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < 7; ++m) s += (scalar * (Pr[m] - Pr[7 + m])) * (-E[m]);     // J^T (-Omega e), Omega = I
                acc += s;
            }
        }
        if (lane < 49) d.H[(int64_t)blk * 49 + lane] = acc;
        else if (lane < 56 && blk < d.na) d.b[(int64_t)blk * 7 + (lane - 49)] = acc;
    }
}

// ------------------------------------------------------------------------------------------------
// factor + solve: ONE workgroup, the elimination tree level by level
// ------------------------------------------------------------------------------------------------
// v = sum over the block pairs of (L_ik L_jk^T)[r][c], pairs in the host's order
__device__ __forceinline__ double eg_pair_sum(const EgDev &d, int blk, int r, int c) {
    double acc = 0.0;
#pragma unroll 4                                 // (the loads of the next pairs issue ahead; the additions stay in pair order)
    for (int q = d.pair_ptr[blk]; q < d.pair_ptr[blk + 1]; ++q) {
        const double *A = d.L + (int64_t)d.pairs[2 * q] * 49 + 7 * r, *B = d.L + (int64_t)d.pairs[2 * q + 1] * 49 + 7 * c;
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 7; ++m) s += A[m] * B[m];
        acc += s;
    }
    return acc;
}

__global__ __launch_bounds__(EG_FT) void eg_factor_solve_kernel(EgDev d) {
    if (d.lm->done) return;
    __shared__ int s_fail;
    __shared__ double s_red[EG_FT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NW = EG_FT / 64;
    const int r = lane < 49 ? lane / 7 : 0, c = lane < 49 ? lane % 7 : 0;
    const double lambda = d.lm->lambda;
    if (threadIdx.x == 0) s_fail = 0;
    __syncthreads();
    // numeric factorisation of H + lambda I (left-looking block Cholesky)
    for (int lv = 0; lv < d.nlev; ++lv) {
        for (int t = d.lvl_ptr[lv] + wave; t < d.lvl_ptr[lv + 1]; t += NW) {            // diagonal blocks of the level's columns
            const int j = d.lvl_col[t];
            double v = d.H[(int64_t)j * 49 + 7 * r + c] + (r == c ? lambda : 0.0);
            v = v - eg_pair_sum(d, j, r, c);
            double A[49], rd[7];
#pragma unroll
            for (int k = 0; k < 49; ++k) A[k] = __shfl(v, k, 64);
            const bool ok = chol_recip<7>(A, rd);
            if (!ok && lane == 0) s_fail = 1;
            if (lane < 49) d.L[(int64_t)j * 49 + lane] = c <= r ? A[lane] : 0.0;
            else if (lane < 56) d.rinv[(int64_t)j * 7 + lane - 49] = rd[lane - 49];
        }
        __syncthreads();
        for (int t = d.off_ptr[lv] + wave; t < d.off_ptr[lv + 1]; t += NW) {            // off-diagonal blocks: (H - sum) L_jj^-T
            const int blk = d.off_blk[t], j = d.blk_col[blk];
            double v = d.H[(int64_t)blk * 49 + 7 * r + c] - eg_pair_sum(d, blk, r, c);
            double row[7];
#pragma unroll
            for (int m = 0; m < 7; ++m) row[m] = __shfl(v, 7 * r + m, 64);
            const double *Lj = d.L + (int64_t)j * 49, *rj = d.rinv + (int64_t)j * 7;
            double X[7];
#pragma unroll
            for (int cc = 0; cc < 7; ++cc) {
                double s = row[cc];
#pragma unroll
                for (int m = 0; m < cc; ++m) s -= X[m] * Lj[7 * cc + m];
                X[cc] = s * rj[cc];
            }
            double out = X[0];
#pragma unroll
            for (int m = 1; m < 7; ++m) out = c == m ? X[m] : out;
            if (lane < 49) d.L[(int64_t)blk * 49 + lane] = out;
        }
        __syncthreads();
    }
    const bool ok = s_fail == 0;
    if (ok) {
        // L y = b, levels upwards: y_j = L_jj^-1 (b_j - sum_k L_jk y_k)
        for (int lv = 0; lv < d.nlev; ++lv) {
            for (int t = d.lvl_ptr[lv] + wave; t < d.lvl_ptr[lv + 1]; t += NW) {
                const int j = d.lvl_col[t];
                const int rr = lane < 7 ? lane : 0;
                double s = d.b[(int64_t)j * 7 + rr];
#pragma unroll 4
                for (int q = d.row_ptr[j]; q < d.row_ptr[j + 1]; ++q) {
                    const double *Lb = d.L + (int64_t)d.row_lst[2 * q] * 49 + 7 * rr, *yk = d.x + (int64_t)d.row_lst[2 * q + 1] * 7;
                    double u = 0.0;
#pragma unroll
                    for (int m = 0; m < 7; ++m) u += Lb[m] * yk[m];
                    s -= u;
                }
                double sv[7], y[7];
#pragma unroll
                for (int m = 0; m < 7; ++m) sv[m] = __shfl(s, m, 64);
                const double *Lj = d.L + (int64_t)j * 49, *rj = d.rinv + (int64_t)j * 7;
#pragma unroll
                for (int i = 0; i < 7; ++i) {
                    double a = sv[i];
#pragma unroll
                    for (int m = 0; m < i; ++m) a -= Lj[7 * i + m] * y[m];
                    y[i] = a * rj[i];
                }
                double out = y[0];
#pragma unroll
                for (int m = 1; m < 7; ++m) out = rr == m ? y[m] : out;
                if (lane < 7) d.x[(int64_t)j * 7 + lane] = out;
            }
            __syncthreads();
        }
        // L^T x = y, levels downwards: x_j = L_jj^-T (y_j - sum_i L_ij^T x_i)
        for (int lv = d.nlev - 1; lv >= 0; --lv) {
            for (int t = d.lvl_ptr[lv] + wave; t < d.lvl_ptr[lv + 1]; t += NW) {
                const int j = d.lvl_col[t];
                const int rr = lane < 7 ? lane : 0;
                double s = d.x[(int64_t)j * 7 + rr];
#pragma unroll 4
                for (int q = d.col_ptr[j]; q < d.col_ptr[j + 1]; ++q) {
                    const double *Lb = d.L + (int64_t)d.col_lst[2 * q] * 49 + rr, *xi = d.x + (int64_t)d.col_lst[2 * q + 1] * 7;
                    double u = 0.0;
#pragma unroll
                    for (int m = 0; m < 7; ++m) u += Lb[7 * m] * xi[m];
                    s -= u;
                }
                double sv[7], xx[7];
#pragma unroll
                for (int m = 0; m < 7; ++m) sv[m] = __shfl(s, m, 64);
                const double *Lj = d.L + (int64_t)j * 49, *rj = d.rinv + (int64_t)j * 7;
#pragma unroll
                for (int i = 6; i >= 0; --i) {
                    double a = sv[i];
#pragma unroll
                    for (int m = i + 1; m < 7; ++m) a -= Lj[7 * m + i] * xx[m];
                    xx[i] = a * rj[i];
                }
                if (d.fix_scale) xx[6] = 0.0;         // VertexSim3Expmap::oplusImpl writes the zero into the solver's x: computeScale sees it
                double out = xx[0];
#pragma unroll
                for (int m = 1; m < 7; ++m) out = rr == m ? xx[m] : out;
                if (lane < 7) d.x[(int64_t)j * 7 + lane] = out;
            }
            __syncthreads();
        }
    }
    // computeScale: sum_j x_j (lambda x_j + b_j), positions and entries in order, threads then waves in index order
    double sc = 0.0;
    if (ok)
        for (int i = threadIdx.x; i < 7 * d.na; i += EG_FT) sc += d.x[i] * (lambda * d.x[i] + d.b[i]);
    sc += lane_xor<1>(sc); sc += lane_xor<2>(sc); sc += lane_xor<4>(sc); sc += lane_xor<8>(sc); sc += lane_xor<16>(sc); sc += lane_xor<32>(sc);
    if (lane == 0) s_red[wave] = sc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < NW; ++k) t += s_red[k];
        d.lm->scale = t;
        d.lm->ok = ok ? 1 : 0;
    }
}

// trial estimates: oplus of the solution into every free vertex, the rest copied
__global__ __launch_bounds__(EG_T) void eg_update_kernel(EgDev d) {
    if (d.lm->done) return;
    const int cur = d.lm->cur;
    const double *src = eg_est(d, cur);
    double *dst = eg_est(d, cur ^ 1);
    for (int v = blockIdx.x * EG_T + threadIdx.x; v < d.n; v += EG_GRID * EG_T) {
        const int p = d.vpos[v];
        Sim3 S = load_sim3(src + 8 * (int64_t)v);
        if (p >= 0) {
            double u[7];
#pragma unroll
            for (int m = 0; m < 7; ++m) u[m] = d.x[(int64_t)p * 7 + m];
            S = sim3_mul(sim3_exp(u), S);
        }
        store_sim3(dst + 8 * (int64_t)v, S);
    }
}

// e'e of every edge at est[k] (trial: k = cur ^ 1; mode 1: the current estimate); the workgroup that finishes last sums them in edge
// order (thread t: edges t, t + EG_T, ...; the lane butterfly; waves in index order) and, for a trial, takes the LM decision
__global__ __launch_bounds__(EG_T) void eg_chi2_kernel(EgDev d, int mode) {
    EgLm &m = *d.lm;
    if (m.done) return;
    const int k = mode ? m.cur : m.cur ^ 1;
    const double *est = eg_est(d, k);
    for (int e = blockIdx.x * EG_T + threadIdx.x; e < d.ne; e += EG_GRID * EG_T) {
        const int vi = d.eij[2 * e], vj = d.eij[2 * e + 1];
        double er[7];
        eg_error(load_sim3(d.meas + 8 * (int64_t)e), load_sim3(est + 8 * (int64_t)vi), sim3_inv(load_sim3(est + 8 * (int64_t)vj)), er);
        double c2 = 0.0;
#pragma unroll
        for (int q = 0; q < 7; ++q) c2 += er[q] * er[q];
        d.chi[e] = c2;
    }
    __shared__ int s_last;
    __shared__ double s_red[EG_T / 64];
    __threadfence();                                  // (every thread's chi before the counter moves)
    __syncthreads();
    if (threadIdx.x == 0) {
        s_last = atomicAdd(d.counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    double s = 0.0;
    for (int e = threadIdx.x; e < d.ne; e += EG_T) s += __builtin_nontemporal_load(d.chi + e);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s += lane_xor<1>(s); s += lane_xor<2>(s); s += lane_xor<4>(s); s += lane_xor<8>(s); s += lane_xor<16>(s); s += lane_xor<32>(s);
    if (lane == 0) s_red[wave] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double chi = 0.0;
    for (int w = 0; w < EG_T / 64; ++w) chi += s_red[w];
    *d.counter = 0u;
    if (mode) { m.current = chi; m.chi_init = chi; return; }
    // OptimizationAlgorithmLevenberg::solve, one trial
    const LmTrial tr = lm_trial(m.current, m.ok ? chi : DBL_MAX, m.scale, m.lambda, m.ni);
    if (tr.accepted) m.cur ^= 1;
    m.rho = tr.rho;
    ++m.qmax; ++m.trials;
    if (tr.rho < 0 && m.qmax < 10) { m.need_lin = 0; return; }          // another trial of the same iteration
    ++m.it;
    if (m.qmax == 10 || tr.rho == 0 || m.it >= m.it_limit) { m.done = 1; return; }
    m.need_lin = 1; m.qmax = 0;
}

// sivo_sim3_correct_points: one thread per point, (float) Swr'.map(Srw.map((double) X))
__global__ __launch_bounds__(EG_T) void eg_correct_points_kernel(const float *xyz, const int *ref, int np, const double *before,
                                                                 const double *after, float *out) {
    const int k = blockIdx.x * EG_T + threadIdx.x;
    if (k >= np) return;
    const float x0 = xyz[3 * (int64_t)k], x1 = xyz[3 * (int64_t)k + 1], x2 = xyz[3 * (int64_t)k + 2];
    const int rf = ref[k];
    if (rf < 0) {
        out[3 * (int64_t)k] = x0; out[3 * (int64_t)k + 1] = x1; out[3 * (int64_t)k + 2] = x2;
        return;
    }
    const Sim3 Srw = load_sim3(before + 8 * (int64_t)rf), Swr = sim3_inv(load_sim3(after + 8 * (int64_t)rf));
    const double X[3] = {(double)x0, (double)x1, (double)x2};
    double Y[3], Z[3];
    sim3_map(Srw, X, Y);
    sim3_map(Swr, Y, Z);
    out[3 * (int64_t)k] = (float)Z[0]; out[3 * (int64_t)k + 1] = (float)Z[1]; out[3 * (int64_t)k + 2] = (float)Z[2];
}

// ------------------------------------------------------------------------------------------------
// host side: ordering and symbolic factorisation (once per call)
// ------------------------------------------------------------------------------------------------
struct EgPlan : SparsePattern {
    int n = 0, ne = 0, n_hoff = 0;
    int64_t nnzL = 0, flops = 0;
    std::vector<int> vpos, own_blk, own_ptr, own_con;
};

static void eg_validate(const uint8_t *fixed, int n, const SivoSim3Edge *e, int ne) {
    if (n < 0 || n > (1 << 22) || ne < 0 || ne > (1 << 24)) throw std::invalid_argument("vertex or edge count out of range");
    if ((n > 0 && !fixed) || (ne > 0 && !e)) throw std::invalid_argument("null argument");
    for (int k = 0; k < ne; ++k) {
        if (e[k].i < 0 || e[k].i >= n || e[k].j < 0 || e[k].j >= n) throw std::invalid_argument("edge vertex index out of range");
        if (e[k].i == e[k].j) throw std::invalid_argument("edge with i == j");
        if (!(e[k].meas[7] > 0.0) || !std::isfinite(e[k].meas[7])) throw std::invalid_argument("the Sim3 scale must be positive");
    }
}

static void eg_plan(const uint8_t *fixed, int n, const SivoSim3Edge *e, int ne, EgPlan &P) {
    P.n = n; P.ne = ne;
    // the variables: free vertices on an edge (g2o's active, non-fixed vertices)
    std::vector<char> on_edge(n, 0);
    for (int k = 0; k < ne; ++k) on_edge[e[k].i] = on_edge[e[k].j] = 1;
    std::vector<int> var;                     // variable -> vertex
    std::vector<int> vid(n, -1);              // vertex -> variable
    for (int v = 0; v < n; ++v)
        if (on_edge[v] && !fixed[v]) { vid[v] = (int)var.size(); var.push_back(v); }
    const int na = (int)var.size();
    P.na = na;
    P.vpos.assign(n, -1);
    if (na == 0) return;
    // ordering (minimum degree, ties to the lower variable = lower vertex index), the blocks of L, the update lists and the levels:
    // sparse_plan.hpp, on the pairs of variables an edge joins
    std::vector<std::pair<int, int>> vp;
    for (int k = 0; k < ne; ++k) {
        const int a = vid[e[k].i], b = vid[e[k].j];
        if (a >= 0 && b >= 0) vp.push_back({a, b});
    }
    sparse_pattern(na, vp, P);
    const int nL = P.nL;
    for (int a = 0; a < na; ++a) P.vpos[var[a]] = P.pos[a];
    // assembly owners: every diagonal block, and every off-diagonal block an edge between two variables touches; contributions in
    // edge order (vertex-0 side first for the diagonal blocks)
    std::vector<std::vector<int>> con(nL);
    auto find_blk = [&](int i, int j) { return P.find_blk(i, j); };
    std::vector<char> hoff(nL, 0);
    for (int k = 0; k < ne; ++k) {
        const int pi = P.vpos[e[k].i], pj = P.vpos[e[k].j];
        if (pi >= 0) con[pi].push_back(k * 4 + 0 * 2 + 0);
        if (pj >= 0) con[pj].push_back(k * 4 + 1 * 2 + 1);
        if (pi >= 0 && pj >= 0) {
            if (pi > pj) { const int b = find_blk(pi, pj); con[b].push_back(k * 4 + 0 * 2 + 1); hoff[b] = 1; }
            else { const int b = find_blk(pj, pi); con[b].push_back(k * 4 + 1 * 2 + 0); hoff[b] = 1; }
        }
    }
    P.own_ptr.push_back(0);
    for (int b = 0; b < nL; ++b) {
        if (b >= na && con[b].empty()) continue;
        P.own_blk.push_back(b);
        P.own_con.insert(P.own_con.end(), con[b].begin(), con[b].end());
        P.own_ptr.push_back((int)P.own_con.size());
    }
    P.n_hoff = 0;
    for (int b = na; b < nL; ++b) P.n_hoff += hoff[b];
    // nnz(L) (lower triangle, scalars) and the flops of one numeric factorisation: 2 x 343 per block product, the 7 x 7 Cholesky,
    // the triangular solve of every off-diagonal block
    P.nnzL = 28 * (int64_t)na + 49 * (int64_t)(nL - na);
    P.flops = 686 * (int64_t)P.pairs.size() / 2 + 161 * (int64_t)na + 343 * (int64_t)(nL - na);
}

// ------------------------------------------------------------------------------------------------
// host side: the device context (one per process, guarded by a mutex: loop closing runs on one thread) and the call
// ------------------------------------------------------------------------------------------------
// (never destroyed: no HIP call from a static destructor at exit)
static std::mutex eg_mu;
static SolverCtx &eg_ctx = *new SolverCtx(false, 256 << 10, 64 << 10, 1 << 20);

static int eg_run(double *siw, const uint8_t *fixed, int n, const SivoSim3Edge *e, int ne, int fix_scale, int iterations, double *chi2,
                  int *iterations_done, int *trials) {
    eg_validate(fixed, n, e, ne);
    if (!siw && n > 0) throw std::invalid_argument("null argument");
    if (iterations < 0 || iterations > 100000) throw std::invalid_argument("iteration count out of range");
    for (int v = 0; v < n; ++v)
        if (!(siw[8 * (size_t)v + 7] > 0.0) || !std::isfinite(siw[8 * (size_t)v + 7])) throw std::invalid_argument("the Sim3 scale must be positive");
    if (chi2) { chi2[0] = 0.0; chi2[1] = 0.0; }
    if (iterations_done) *iterations_done = 0;
    if (trials) *trials = 0;
    if (n == 0) return SIVO_OK;
    require_device();
    if (ne == 0) return SIVO_OK;                                  // (no edge: no active vertex, chi2 = 0, nothing to do)
    EgPlan P;
    eg_plan(fixed, n, e, ne, P);
    std::vector<int> eij(2 * (size_t)ne);
    std::vector<double> meas(8 * (size_t)ne);
    for (int k = 0; k < ne; ++k) {
        eij[2 * (size_t)k] = e[k].i; eij[2 * (size_t)k + 1] = e[k].j;
        std::memcpy(meas.data() + 8 * (size_t)k, e[k].meas, 64);
    }
    const int na = P.na, nL = P.nL;
    EgLm lm0{};
    lm0.lambda = 1e-16;                       // setUserLambdaInit(1e-16): computeLambdaInit returns it at iteration 0
    lm0.ni = 2; lm0.need_lin = 1; lm0.it_limit = iterations;
    // staging: the inputs and the initial state (one copy up), the device-only work arrays (one memset)
    EgDev d;
    Layout L;
    L.copy(d.est0, siw, 64 * (size_t)n);
    L.copy(d.vpos, P.vpos.data(), 4 * P.vpos.size()); L.copy(d.eij, eij.data(), 4 * eij.size()); L.copy(d.meas, meas.data(), 8 * meas.size());
    L.copy(d.own_blk, P.own_blk.data(), 4 * P.own_blk.size()); L.copy(d.own_ptr, P.own_ptr.data(), 4 * P.own_ptr.size());
    L.copy(d.own_con, P.own_con.data(), 4 * P.own_con.size());
    L.copy(d.lvl_ptr, P.lvl_ptr.data(), 4 * P.lvl_ptr.size()); L.copy(d.lvl_col, P.lvl_col.data(), 4 * P.lvl_col.size());
    L.copy(d.off_ptr, P.off_ptr.data(), 4 * P.off_ptr.size()); L.copy(d.off_blk, P.off_blk.data(), 4 * P.off_blk.size());
    L.copy(d.blk_col, P.blk_col.data(), 4 * P.blk_col.size());
    L.copy(d.pair_ptr, P.pair_ptr.data(), 4 * P.pair_ptr.size()); L.copy(d.pairs, P.pairs.data(), 4 * P.pairs.size());
    L.copy(d.row_ptr, P.row_ptr.data(), 4 * P.row_ptr.size()); L.copy(d.row_lst, P.row_lst.data(), 4 * P.row_lst.size());
    L.copy(d.col_ptr, P.col_ptr.data(), 4 * P.col_ptr.size()); L.copy(d.col_lst, P.col_lst.data(), 4 * P.col_lst.size());
    L.copy(d.lm, &lm0, sizeof(EgLm));
    L.zero(d.est1, 64 * (size_t)n); L.zero(d.counter, 4);
    L.zero(d.H, 49 * 8 * (size_t)nL);                            // (the fill blocks stay zero)
    L.zero(d.pert, 224 * 8 * (size_t)na); L.zero(d.errs, EG_NERR * 7 * 8 * (size_t)ne); L.zero(d.chi, 8 * (size_t)ne);
    L.zero(d.b, 7 * 8 * (size_t)na); L.zero(d.L, 49 * 8 * (size_t)nL); L.zero(d.rinv, 7 * 8 * (size_t)na); L.zero(d.x, 7 * 8 * (size_t)na);
    d.n = n; d.ne = ne; d.na = na; d.nlev = P.nlev; d.n_own = (int)P.own_blk.size(); d.fix_scale = fix_scale ? 1 : 0;
    std::lock_guard<std::mutex> lock(eg_mu);
    SolverCtx &c = eg_ctx;
    c.bind();
    L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.staged()));
    EgLm *hl = (EgLm *)c.out.reserve(sizeof(EgLm));
    hipStream_t st = c.stream;
    L.send(st);
    // the chi2 of the input (mode 1: current = chi_init), then the steps
    hipLaunchKernelGGL(eg_chi2_kernel, dim3(EG_GRID), dim3(EG_T), 0, st, d, 1);
    SIVO_HIP(hipGetLastError());
    // (every vertex on an edge fixed: g2o's optimize() finds nothing to optimise and returns; at most 10 trials per iteration)
    const int max_steps = na == 0 ? 0 : iterations * 10;
    int steps = 0;
    const int batch = 8;
    for (;;) {
        SIVO_HIP(hipMemcpyAsync(hl, d.lm, sizeof(EgLm), hipMemcpyDeviceToHost, st));
        SIVO_HIP(hipStreamSynchronize(st));
        if (hl->done || steps >= max_steps) break;
        for (int s = 0; s < batch && steps < max_steps; ++s, ++steps) {
            hipLaunchKernelGGL(eg_perturb_kernel, dim3(EG_GRID), dim3(EG_T), 0, st, d);
            hipLaunchKernelGGL(eg_errors_kernel, dim3(EG_GRID), dim3(EG_T), 0, st, d);
            hipLaunchKernelGGL(eg_assemble_kernel, dim3(EG_GRID), dim3(EG_T), 0, st, d);
            hipLaunchKernelGGL(eg_factor_solve_kernel, dim3(1), dim3(EG_FT), 0, st, d);
            hipLaunchKernelGGL(eg_update_kernel, dim3(EG_GRID), dim3(EG_T), 0, st, d);
            hipLaunchKernelGGL(eg_chi2_kernel, dim3(EG_GRID), dim3(EG_T), 0, st, d, 0);
        }
        SIVO_HIP(hipGetLastError());
    }
    // the current estimate back
    const int cur = hl->cur;
    SIVO_HIP(hipMemcpyAsync(siw, cur ? d.est1 : d.est0, 64 * (size_t)n, hipMemcpyDeviceToHost, st));
    SIVO_HIP(hipStreamSynchronize(st));
    if (chi2) { chi2[0] = hl->chi_init; chi2[1] = hl->current; }
    if (iterations_done) *iterations_done = hl->it;
    if (trials) *trials = hl->trials;
    return SIVO_OK;
}

static int eg_correct(const float *xyz, const int32_t *ref, int np, const double *before, const double *after, int n, float *out) {
    if (np < 0 || np > (1 << 26) || n < 0 || n > (1 << 22)) throw std::invalid_argument("count out of range");
    if (np > 0 && (!xyz || !ref || !out)) throw std::invalid_argument("null argument");
    if (n > 0 && (!before || !after)) throw std::invalid_argument("null argument");
    for (int v = 0; v < n; ++v)
        if (!(before[8 * (size_t)v + 7] > 0.0) || !(after[8 * (size_t)v + 7] > 0.0) || !std::isfinite(before[8 * (size_t)v + 7]) ||
            !std::isfinite(after[8 * (size_t)v + 7]))
            throw std::invalid_argument("the Sim3 scale must be positive");
    for (int k = 0; k < np; ++k)
        if (ref[k] < -1 || ref[k] >= n) throw std::invalid_argument("reference index out of range");
    if (np == 0) return SIVO_OK;
    require_device();
    const float *d_xyz; const int *d_ref; const double *d_before, *d_after; float *d_out;
    Layout L;
    L.copy(d_xyz, xyz, 12 * (size_t)np); L.copy(d_ref, ref, 4 * (size_t)np);
    L.copy(d_before, before, 64 * (size_t)n); L.copy(d_after, after, 64 * (size_t)n);
    L.take(d_out, 12 * (size_t)np);
    std::lock_guard<std::mutex> lock(eg_mu);
    SolverCtx &c = eg_ctx;
    c.bind();
    L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.staged()));
    char *h_out = c.out.reserve(12 * (size_t)np);
    L.send(c.stream);
    hipLaunchKernelGGL(eg_correct_points_kernel, dim3((np + EG_T - 1) / EG_T), dim3(EG_T), 0, c.stream, d_xyz, d_ref, np, d_before, d_after, d_out);
    SIVO_HIP(hipGetLastError());
    SIVO_HIP(hipMemcpyAsync(h_out, d_out, 12 * (size_t)np, hipMemcpyDeviceToHost, c.stream));
    SIVO_HIP(hipStreamSynchronize(c.stream));
    std::memcpy(out, h_out, 12 * (size_t)np);
    return SIVO_OK;
}

}  // namespace sivo

using namespace sivo;

extern "C" int sivo_essential_graph_optimize(double *siw, const uint8_t *fixed, int n, const SivoSim3Edge *e, int ne, int fix_scale,
                                             int iterations, double *chi2, int *iterations_done, int *trials) {
    return guarded([&] { return eg_run(siw, fixed, n, e, ne, fix_scale, iterations, chi2, iterations_done, trials); });
}

extern "C" int sivo_essential_graph_analyze(const uint8_t *fixed, int n, const SivoSim3Edge *e, int ne, int64_t out[6]) {
    return guarded([&] {
        if (!out) throw std::invalid_argument("null argument");
        eg_validate(fixed, n, e, ne);
        EgPlan P;
        eg_plan(fixed, n, e, ne, P);
        out[0] = P.na; out[1] = P.nL - P.na; out[2] = P.nnzL; out[3] = P.flops; out[4] = P.nlev; out[5] = P.n_hoff;
        return SIVO_OK;
    });
}

extern "C" int sivo_sim3_correct_points(const float *xyz, const int32_t *ref, int np, const double *siw_before, const double *siw_after,
                                        int n, float *out) {
    return guarded([&] { return eg_correct(xyz, ref, np, siw_before, siw_after, n, out); });
}
