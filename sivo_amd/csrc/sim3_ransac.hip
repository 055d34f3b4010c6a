// sim3_ransac.hip — Sim3Solver's RANSAC (reference src/orbslam/Sim3Solver.cc), the first step of LoopClosing::ComputeSim3
// (LoopClosing.cc:281-307): Horn's closed form on a sample of three correspondences (ComputeSim3, :224-349), then the two-way
// reprojection test of every correspondence (CheckInliers / Project, :352-409), up to 300 times per loop candidate.  Every
// (candidate, hypothesis, pair) is independent of every other: ONE launch evaluates every hypothesis of every candidate
// (sivo_sim3_ransac_batch), the sequential bookkeeping of iterate() (:143-208: the running best, the first acceptance) is two scans
// over the counts, done on the host in the ABI.
//
// Arithmetic: the reference works on CV_32F cv::Mats; which intermediate is float and which double follows from OpenCV's
// gemm / convertTo / dot rules as sivo_amd/api/compat/cv_min.hpp states them, and this file follows Sim3Solver.cc operation for
// operation under those rules (an expression no stated rule covers carries the OpenCV rule it follows in a comment).  Two
// substitutions, neither pinned (OpenCV is absent): cv::eigen is a cyclic Jacobi in double on the float N matrix
// (RS_SWEEPS sweeps, pairs in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), the eigenvector of the largest eigenvalue, ties to
// the lowest index), and atan2 + cv::Rodrigues is the rotation matrix of the quaternion formed directly in double and rounded
// once to float.  Only + - * / sqrt and float / double conversions are used, each correctly rounded under the library's flags
// (no contraction): tests/sim3_ransac_restatement.py restates the kernel in numpy and is compared bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "common.hpp"
#include "solver_host.hpp"

#pragma clang fp contract(off)

namespace sivo {

// ------------------------------------------------------------------------------------------------
// the kernel
//
//   * one wave per hypothesis, RS_WAVES hypotheses of ONE problem per workgroup;
//   * the workgroup stages its problem's pairs in LDS up to RS_CAP = 1024 of them (12 floats each: X1c, X2c, the two thresholds
//     and the pair's projections into its own images, FromCameraToImage, computed once; the launch asks LDS for
//     min(max n, RS_CAP) pairs); pairs beyond that are read from memory and their own projections recomputed, the same
//     operations on the same values;
//   * every lane forms the hypothesis' T12 / T21 from the triple (uniform work: no broadcast, no barrier);
//   * the wave walks the pairs 64 at a time: a ballot is one word of inlier_bits, its popcount goes into the count.
// ------------------------------------------------------------------------------------------------
constexpr int RS_WAVES = 4, RS_THREADS = 64 * RS_WAVES, RS_CAP = 1024, RS_REC = 12, RS_SWEEPS = 8;
constexpr size_t rs_lds_bytes(int cap) { return (size_t)cap * RS_REC * 4; }
static_assert(rs_lds_bytes(RS_CAP) <= 64 * 1024, "the LDS copy of the pairs stays below the default dynamic LDS limit");

struct RsProb {                // one problem as staged on the device
    float k1[4], k2[4];
    int64_t pair_off, hyp_off, word_off;   // first pair / hypothesis / inlier word of the problem in the batch's arrays
    int32_t n, n_hyp, fix_scale, words;    // words = ceil(n / 64)
};
struct RsBlock { int32_t prob, first; };   // workgroup -> its problem and the first of its RS_WAVES hypotheses

struct RsArgs {
    const RsProb *prob;
    const RsBlock *block;
    const SivoSim3Pair *pairs;
    const int32_t *triples;    // 3 per hypothesis
    int32_t *count;            // 1 per hypothesis
    float *T;                  // 13 per hypothesis
    uint64_t *bits;            // words per hypothesis
    int lds_cap;
};

// One element of cv::gemm's small-matrix path (cv_min.hpp: inner dimension 3, no transposed operand): the dot product summed left
// to right in float, then (float)(t * alpha + c) in double, c = C's element times beta (0.0 without C).
__device__ __forceinline__ float rs_gemm3(float a0, float a1, float a2, float b0, float b1, float b2, double alpha, double c) {
    float t = a0 * b0;
    t = t + a1 * b1;
    t = t + a2 * b2;
    return (float)((double)t * alpha + c);
}

// FromCameraToImage (:411-429) / the tail of Project (:403-407)
__device__ __forceinline__ void rs_to_image(float X, float Y, float Z, const float (&K)[4], float &u, float &v) {
    const float invz = 1 / Z;
    const float x = X * invz;
    const float y = Y * invz;
    u = K[0] * x + K[2];
    v = K[1] * y + K[3];
}

// Project (:387-409): P3Dc = Rcw * X + tcw, one gemm with C = tcw and beta = 1
__device__ __forceinline__ void rs_project(const float (&R)[9], const float (&t)[3], const float (&X)[3], const float (&K)[4], float &u,
                                           float &v) {
    const float x = rs_gemm3(R[0], R[1], R[2], X[0], X[1], X[2], 1.0, (double)t[0] * 1.0);
    const float y = rs_gemm3(R[3], R[4], R[5], X[0], X[1], X[2], 1.0, (double)t[1] * 1.0);
    const float z = rs_gemm3(R[6], R[7], R[8], X[0], X[1], X[2], 1.0, (double)t[2] * 1.0);
    rs_to_image(x, y, z, K, u, v);
}

template <int P, int Q>
__device__ __forceinline__ void rs_jacobi_rot(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq != 0.0) {          // (a NaN enters: it propagates as every other value does)
        const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0);
        const double s = t * c;
        A[P][P] = A[P][P] - t * apq;
        A[Q][Q] = A[Q][Q] + t * apq;
        A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r == P || r == Q) continue;
            const double arp = A[r][P], arq = A[r][Q];
            A[r][P] = c * arp - s * arq; A[P][r] = A[r][P];
            A[r][Q] = s * arp + c * arq; A[Q][r] = A[r][Q];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double vrp = V[r][P], vrq = V[r][Q];
            V[r][P] = c * vrp - s * vrq;
            V[r][Q] = s * vrp + c * vrq;
        }
    }
}

struct RsHyp { float R[9], t[3], s, sR[9], sRinv[9], tinv[3]; };

// ComputeCentroid (:215-222): cv::reduce(P, C, 1, CV_REDUCE_SUM) on three columns is reduceC_<float, float, OpAdd>: a0 = c0,
// a1 = c1, a0 += c2, a0 += a1, all float; C / P.cols is convertTo with the factor 1.0 / 3 narrowed to float.
__device__ __forceinline__ void rs_centroid(const float (&P)[3][3], float (&Pr)[3][3], float (&C)[3]) {
    const float third = (float)(1.0 / 3);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float a0 = P[r][0] + P[r][2];
        a0 = a0 + P[r][1];
        C[r] = a0 * third;
#pragma unroll
        for (int i = 0; i < 3; ++i) Pr[r][i] = P[r][i] - C[r];
    }
}

// ComputeSim3 (:224-349); P1 / P2: row = coordinate, column = sample
__device__ __forceinline__ void rs_horn(const float (&P1)[3][3], const float (&P2)[3][3], bool fix_scale, RsHyp &h) {
    float Pr1[3][3], Pr2[3][3], O1[3], O2[3];
    rs_centroid(P1, Pr1, O1);
    rs_centroid(P2, Pr2, O2);
    // M = Pr2 * Pr1.t(): a transposed operand, products and sum in double, (float)(alpha * sum + c)
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += (double)Pr2[i][k] * (double)Pr1[j][k];
            M[i][j] = (float)(1.0 * s + 0.0);
        }
    // N (:251-260): the right-hand sides are float expressions (C++ evaluates float + float in float) assigned to doubles and
    // stored into a CV_32F matrix: the float values
    const float N11 = M[0][0] + M[1][1] + M[2][2];
    const float N12 = M[1][2] - M[2][1];
    const float N13 = M[2][0] - M[0][2];
    const float N14 = M[0][1] - M[1][0];
    const float N22 = M[0][0] - M[1][1] - M[2][2];
    const float N23 = M[0][1] + M[1][0];
    const float N24 = M[2][0] + M[0][2];
    const float N33 = -M[0][0] + M[1][1] - M[2][2];
    const float N34 = M[1][2] + M[2][1];
    const float N44 = -M[0][0] - M[1][1] + M[2][2];
    // cv::eigen (unpinned): cyclic Jacobi in double
    double A[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34}, {N14, N24, N34, N44}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma unroll 1
    for (int sweep = 0; sweep < RS_SWEEPS; ++sweep) {
        rs_jacobi_rot<0, 1>(A, V); rs_jacobi_rot<0, 2>(A, V); rs_jacobi_rot<0, 3>(A, V);
        rs_jacobi_rot<1, 2>(A, V); rs_jacobi_rot<1, 3>(A, V); rs_jacobi_rot<2, 3>(A, V);
    }
    double best = A[0][0], e[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > best) { best = A[k][k]; e[0] = V[0][k]; e[1] = V[1][k]; e[2] = V[2][k]; e[3] = V[3][k]; }
    // evec is CV_32F: the quaternion (w, x, y, z) as floats.  atan2 + Rodrigues (unpinned): angle 2 atan2(|v|, w) about v / |v| is the
    // rotation of the quaternion normalised, formed in double and rounded once.  |v| == 0 makes the reference's axis 0 / 0 and
    // its matrix NaN: the factor v2 / v2 (exactly 1 otherwise) does the same.
    const double w = (double)(float)e[0], x = (double)(float)e[1], y = (double)(float)e[2], z = (double)(float)e[3];
    const double xx = x * x, yy = y * y, zz = z * z, ww = w * w;
    const double v2 = xx + yy + zz, n2 = ww + v2, f = v2 / v2;
    const double Rd[9] = {(ww + xx - yy - zz) / n2 * f, 2.0 * (x * y - w * z) / n2 * f, 2.0 * (x * z + w * y) / n2 * f,
                          2.0 * (x * y + w * z) / n2 * f, (ww - xx + yy - zz) / n2 * f, 2.0 * (y * z - w * x) / n2 * f,
                          2.0 * (x * z - w * y) / n2 * f, 2.0 * (y * z + w * x) / n2 * f, (ww - xx - yy + zz) / n2 * f};
#pragma unroll
    for (int i = 0; i < 9; ++i) h.R[i] = (float)Rd[i];
    // P3 = mR12i * Pr2 (:304): the small-matrix path
    float P3[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) P3[i][j] = rs_gemm3(h.R[3 * i], h.R[3 * i + 1], h.R[3 * i + 2], Pr2[0][j], Pr2[1][j], Pr2[2][j], 1.0, 0.0);
    if (!fix_scale) {
        // nom = Pr1.dot(P3) in double; cv::pow(P3, 2) squares in float, den sums the floats in a double (:309-321)
        double nom = 0.0, den = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                nom += (double)Pr1[i][j] * (double)P3[i][j];
                den += P3[i][j] * P3[i][j];
            }
        h.s = (float)(nom / den);
    } else {
        h.s = 1.0f;
    }
    // mt12i = O1 - ms12i * mR12i * O2 (:328): MatOp_GEMM::subtract folds `C - alpha A B` into ONE gemm with alpha = -ms12i, beta = 1
#pragma unroll
    for (int i = 0; i < 3; ++i)
        h.t[i] = rs_gemm3(h.R[3 * i], h.R[3 * i + 1], h.R[3 * i + 2], O2[0], O2[1], O2[2], -(double)h.s, (double)O1[i] * 1.0);
    // sR = ms12i * mR12i; sRinv = (1.0 / ms12i) * mR12i.t(): the factor narrowed to float (:335, :344)
    const float sinv = (float)(1.0 / (double)h.s);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            h.sR[3 * i + j] = h.R[3 * i + j] * (float)(double)h.s;
            h.sRinv[3 * i + j] = h.R[3 * j + i] * sinv;
        }
    // tinv = -sRinv * mt12i (:347): the small-matrix path with alpha = -1
#pragma unroll
    for (int i = 0; i < 3; ++i)
        h.tinv[i] = rs_gemm3(h.sRinv[3 * i], h.sRinv[3 * i + 1], h.sRinv[3 * i + 2], h.t[0], h.t[1], h.t[2], -1.0, 0.0);
}

// CheckInliers (:352-372) for one pair: dist.dot(dist) in double narrowed to float, compared as floats (the unsigned long threshold
// converts to float); a NaN error is not an inlier
__device__ __forceinline__ bool rs_inlier(const RsHyp &h, const float (&K1)[4], const float (&K2)[4], const float (&X1)[3],
                                          const float (&X2)[3], float max1, float max2, float u1, float v1, float u2, float v2) {
    float pu, pv;
    rs_project(h.sR, h.t, X2, K1, pu, pv);                     // vP2im1
    const float a0 = u1 - pu, a1 = v1 - pv;
    rs_project(h.sRinv, h.tinv, X1, K2, pu, pv);               // vP1im2
    const float b0 = pu - u2, b1 = pv - v2;
    const float err1 = (float)((double)a0 * (double)a0 + (double)a1 * (double)a1);
    const float err2 = (float)((double)b0 * (double)b0 + (double)b1 * (double)b1);
    return err1 < max1 && err2 < max2;
}

__global__ __launch_bounds__(RS_THREADS) void sim3_ransac_kernel(RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];             // [RS_REC][cap]
    const int cap = a.lds_cap;
    const RsBlock blk = a.block[blockIdx.x];
    const RsProb &pr = a.prob[blk.prob];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = pr.n;
    const SivoSim3Pair *const pairs = a.pairs + pr.pair_off;
    float K1[4], K2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { K1[i] = pr.k1[i]; K2[i] = pr.k2[i]; }
    for (int p = tid; p < n && p < cap; p += RS_THREADS) {
        const SivoSim3Pair q = pairs[p];
        float *s = rs_lds + p;
        s[0] = q.x1c[0]; s[cap] = q.x1c[1]; s[2 * cap] = q.x1c[2]; s[3 * cap] = q.x2c[0]; s[4 * cap] = q.x2c[1]; s[5 * cap] = q.x2c[2];
        s[6 * cap] = q.max_err1; s[7 * cap] = q.max_err2;
        rs_to_image(q.x1c[0], q.x1c[1], q.x1c[2], K1, s[8 * cap], s[9 * cap]);        // mvP1im1
        rs_to_image(q.x2c[0], q.x2c[1], q.x2c[2], K2, s[10 * cap], s[11 * cap]);      // mvP2im2
    }
    __syncthreads();
    const int hl = blk.first + wave;                                // the wave's hypothesis within the problem
    if (hl >= pr.n_hyp) return;
    const int64_t hg = pr.hyp_off + hl;
    const int32_t *tri = a.triples + 3 * hg;
    float P1[3][3], P2[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                   // (indices checked by the host: 0 <= tri[i] < n)
        const SivoSim3Pair q = pairs[tri[i]];
#pragma unroll
        for (int r = 0; r < 3; ++r) { P1[r][i] = q.x1c[r]; P2[r][i] = q.x2c[r]; }
    }
    RsHyp h;
    rs_horn(P1, P2, pr.fix_scale != 0, h);
    uint64_t *const bits = a.bits + pr.word_off + (int64_t)hl * pr.words;
    int count = 0;
    // the LDS copy first, then the pairs beyond it (two loops: one load path each, as in sim3.hip)
    const int n_lds = n < cap ? n : cap;
    for (int base = 0; base < n_lds; base += 64) {
        const int p = base + lane;
        bool in = false;
        if (p < n_lds) {
            const float *s = rs_lds + p;
            const float X1[3] = {s[0], s[cap], s[2 * cap]}, X2[3] = {s[3 * cap], s[4 * cap], s[5 * cap]};
            in = rs_inlier(h, K1, K2, X1, X2, s[6 * cap], s[7 * cap], s[8 * cap], s[9 * cap], s[10 * cap], s[11 * cap]);
        }
        const uint64_t word = __ballot(in);
        if (lane == 0) bits[base >> 6] = word;
        count += __popcll(word);
    }
    for (int base = n_lds; base < n; base += 64) {                  // (RS_CAP is a multiple of 64: `base` stays word-aligned)
        const int p = base + lane;
        bool in = false;
        if (p < n) {
            const SivoSim3Pair q = pairs[p];
            float u1, v1, u2, v2;
            rs_to_image(q.x1c[0], q.x1c[1], q.x1c[2], K1, u1, v1);
            rs_to_image(q.x2c[0], q.x2c[1], q.x2c[2], K2, u2, v2);
            in = rs_inlier(h, K1, K2, q.x1c, q.x2c, q.max_err1, q.max_err2, u1, v1, u2, v2);
        }
        const uint64_t word = __ballot(in);
        if (lane == 0) bits[base >> 6] = word;
        count += __popcll(word);
    }
    if (lane == 0) {
        a.count[hg] = count;
        // (sign and payload of a NaN depend on the machine that produced it: every NaN is stored as the quiet NaN 0x7FC00000)
        const float v[13] = {h.R[0], h.R[1], h.R[2], h.R[3], h.R[4], h.R[5], h.R[6], h.R[7], h.R[8], h.t[0], h.t[1], h.t[2], h.s};
        float *o = a.T + 13 * hg;
#pragma unroll
        for (int i = 0; i < 13; ++i) o[i] = v[i] != v[i] ? __uint_as_float(0x7FC00000u) : v[i];
    }
}
static_assert(RS_CAP % 64 == 0, "a ballot word never straddles the LDS cap");

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int ransac_run(SivoSim3RansacProblem *probs, int k) {
    if (k < 0 || k > (1 << 16)) throw std::invalid_argument("problem count out of range");
    if (k > 0 && !probs) throw std::invalid_argument("null argument");
    int64_t pairs = 0, hyps = 0, words = 0, blocks = 0;
    int max_n = 0;
    for (int i = 0; i < k; ++i) {
        const SivoSim3RansacProblem &p = probs[i];
        if (p.n < 0 || p.n > (1 << 22)) throw std::invalid_argument("pair count out of range");
        if (p.n_hyp < 0 || p.n_hyp > (1 << 20)) throw std::invalid_argument("hypothesis count out of range");
        if (p.n && !p.pairs) throw std::invalid_argument("null argument");
        if (p.n_hyp) {
            if (p.n < 3) throw std::invalid_argument("a hypothesis needs three pairs");
            if (!p.triples || !p.count || !p.T || !p.inlier_bits) throw std::invalid_argument("null argument");
            for (int64_t h = 0; h < p.n_hyp; ++h) {
                const int32_t *t = p.triples + 3 * h;
                if (t[0] < 0 || t[0] >= p.n || t[1] < 0 || t[1] >= p.n || t[2] < 0 || t[2] >= p.n)
                    throw std::invalid_argument("triple index out of range");
                if (t[0] == t[1] || t[0] == t[2] || t[1] == t[2]) throw std::invalid_argument("a triple repeats an index");
            }
            pairs += p.n; hyps += p.n_hyp; words += (int64_t)p.n_hyp * cdiv(p.n, 64); blocks += cdiv(p.n_hyp, RS_WAVES);
            max_n = std::max(max_n, p.n);
        }
    }
    if (pairs > (int64_t)1 << 26 || hyps > (int64_t)1 << 22 || words > (int64_t)1 << 27) throw std::invalid_argument("batch too large");
    for (int i = 0; i < k; ++i) { probs[i].first_accept = -1; probs[i].best = -1; }
    if (hyps == 0) return SIVO_OK;
    require_device();
    // the loop-closing thread evaluates its candidates: one pinned buffer for the upload and the results, kept per thread
    static thread_local SolverCtx c(true, 256 << 10, 0, 256 << 10);
    c.bind();
    // upload: the problem headers, the workgroup table, then every problem's pairs and triples back to back (staged in place);
    // results: count, T, inlier words per hypothesis.  One copy each way, one launch, one synchronisation.
    RsArgs a;
    Layout L;
    L.copy(a.prob, nullptr, sizeof(RsProb) * (size_t)k);
    L.copy(a.block, nullptr, sizeof(RsBlock) * (size_t)blocks);
    L.copy(a.pairs, nullptr, sizeof(SivoSim3Pair) * (size_t)pairs);
    L.copy(a.triples, nullptr, 12 * (size_t)hyps);
    L.take(a.count, 4 * (size_t)hyps); L.take(a.T, 52 * (size_t)hyps); L.take(a.bits, 8 * (size_t)words);
    L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
    RsProb *hp = L.host(a.prob);
    RsBlock *hb = L.host(a.block);
    SivoSim3Pair *hpair = L.host(a.pairs);
    int32_t *htri = L.host(a.triples);
    int64_t po = 0, ho = 0, wo = 0, bo = 0;
    for (int i = 0; i < k; ++i) {
        const SivoSim3RansacProblem &p = probs[i];
        RsProb &q = hp[i];
        std::memcpy(q.k1, p.k1, sizeof q.k1); std::memcpy(q.k2, p.k2, sizeof q.k2);
        q.pair_off = po; q.hyp_off = ho; q.word_off = wo;
        q.n = p.n; q.n_hyp = p.n_hyp; q.fix_scale = p.fix_scale ? 1 : 0; q.words = cdiv(p.n, 64);
        if (!p.n_hyp) continue;
        std::memcpy(hpair + po, p.pairs, sizeof(SivoSim3Pair) * (size_t)p.n);
        std::memcpy(htri + 3 * ho, p.triples, 12 * (size_t)p.n_hyp);
        for (int f = 0; f < p.n_hyp; f += RS_WAVES) hb[bo++] = RsBlock{i, f};
        po += p.n; ho += p.n_hyp; wo += (int64_t)p.n_hyp * q.words;
    }
    a.lds_cap = std::max(1, std::min(max_n, RS_CAP));
    L.send(c.stream);
    hipLaunchKernelGGL(sim3_ransac_kernel, dim3((unsigned)blocks), dim3(RS_THREADS), rs_lds_bytes(a.lds_cap), c.stream, a);
    SIVO_HIP(hipGetLastError());
    SIVO_HIP(hipMemcpyAsync(L.host(a.count), a.count, L.results(), hipMemcpyDeviceToHost, c.stream));
    SIVO_HIP(hipStreamSynchronize(c.stream));
    const int32_t *cnt = L.host(a.count);
    const float *T = L.host(a.T);
    const uint64_t *bits = L.host(a.bits);
    for (int i = 0; i < k; ++i) {
        SivoSim3RansacProblem &p = probs[i];
        if (!p.n_hyp) continue;
        const RsProb &q = hp[i];
        std::memcpy(p.count, cnt + q.hyp_off, 4 * (size_t)p.n_hyp);
        std::memcpy(p.T, T + 13 * q.hyp_off, 52 * (size_t)p.n_hyp);
        std::memcpy(p.inlier_bits, bits + q.word_off, 8 * (size_t)p.n_hyp * (size_t)q.words);
        // iterate() (:186-200) over the counts: mnBestInliers starts at 0 and is replaced under >=, the first count above
        // min_inliers returns
        int best_count = 0;
        for (int h = 0; h < p.n_hyp; ++h) {
            if (p.count[h] >= best_count) { best_count = p.count[h]; p.best = h; }
            if (p.first_accept < 0 && p.count[h] > p.min_inliers) p.first_accept = h;
        }
    }
    return SIVO_OK;
}

}  // namespace sivo

using namespace sivo;

extern "C" int sivo_sim3_ransac_batch(SivoSim3RansacProblem *problems, int n_problems) {
    return guarded([&] { return ransac_run(problems, n_problems); });
}

extern "C" int sivo_sim3_ransac(SivoSim3RansacProblem *problem) {
    return guarded([&] {
        if (!problem) throw std::invalid_argument("null argument");
        return ransac_run(problem, 1);
    });
}
