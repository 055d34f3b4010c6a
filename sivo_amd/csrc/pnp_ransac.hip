// pnp_ransac.hip — PnPsolver's EPnP RANSAC (reference src/orbslam/PnPsolver.cc), the step of Tracking::Relocalization
// (Tracking.cc:1279-1330) between SearchByBoW and PoseOptimization: EPnP on a sample of four correspondences (compute_pose, :482-531),
// then the reprojection test of every correspondence (CheckInliers, :318-347), up to 300 times per candidate keyframe, and a full-size
// EPnP on the inliers of the running best (Refine, :271-315).  Every (candidate, hypothesis, correspondence) is independent of every
// other: ONE launch evaluates every hypothesis of every candidate (pnp_hyp_kernel); the sequential bookkeeping of iterate() (:198-253)
// is a scan over the counts, done on the host in the ABI, which marks the records: the hypotheses at which the running best is replaced.
// Refine is a pure function of mvbBestInliers, which changes only at a record: a second launch refines every record of every candidate
// (pnp_refine_kernel).
//
// Arithmetic: pnp_epnp.hpp restates the reference in double, operation for operation, and names the substitutions for cvSVD, cvSolve,
// cvInvert and cvMulTransposed (OpenCV is absent, none of them is pinned: DESIGN 3.6d, 5).  Only + - * / sqrt, comparisons and float /
// double conversions, each correctly rounded under the library's flags (no contraction): tests/pnp_ransac_restatement.py restates both
// kernels in numpy and is compared bit for bit.  A NaN in a stored pose is the quiet NaN 0x7FF8000000000000.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "common.hpp"
#include "solver_host.hpp"

#pragma clang fp contract(off)

#include "pnp_epnp.hpp"

namespace sivo {

// ------------------------------------------------------------------------------------------------
// the kernels
//
//   * one wave per EPnP: PN_WAVES hypotheses of ONE problem per workgroup (pnp_hyp_kernel), one refinement per workgroup of one wave
//     (pnp_refine_kernel);
//   * the 12 x 12 M'M, its eigenvectors and every other small matrix of the solve live in LDS (PnpWork, one per wave); a Jacobi
//     rotation's rows are spread over the lanes, the reductions over the correspondences have one lane per output entry, the serial
//     algebra runs on lane 0 (pnp_epnp.hpp).  The team's barrier is the workgroup's: every wave of a workgroup runs the same sequence
//     of barriers (the trip counts depend on nothing but constants), an idle wave of the last workgroup repeats its problem's last
//     hypothesis and writes nothing;
//   * the hypothesis kernel stages its problem's correspondences in LDS up to PN_CAP = 1024 of them (6 floats each); those beyond, and
//     all of them in the refine kernel, are read from memory: the same operations on the same values;
//   * the wave walks the correspondences 64 at a time: a ballot is one word of inlier_bits, its popcount goes into the count.
// ------------------------------------------------------------------------------------------------
constexpr int PN_WAVES = 4, PN_THREADS = 64 * PN_WAVES, PN_CAP = 1024, PN_REC = 6;
constexpr size_t pn_lds_bytes(int cap) { return (size_t)cap * PN_REC * 4; }
static_assert(pn_lds_bytes(PN_CAP) + PN_WAVES * sizeof(PnpWork) <= 64 * 1024, "the LDS copy of the points and the workspaces stay below 64 KiB");
static_assert(PN_CAP % 64 == 0, "a ballot word never straddles the LDS cap");

struct PnpWaveTeam {
    int lane;
    static constexpr int size = 64;
    __device__ void sync() const { __syncthreads(); }
};

struct PnProb {                // one problem as staged on the device
    float K[4];
    int64_t pt_off, hyp_off, word_off;     // first point / hypothesis / inlier word of the problem in the batch's arrays
    int32_t n, n_hyp, words, pad_;         // words = ceil(n / 64)
};
struct PnBlock { int32_t prob, first; };   // workgroup -> its problem and the first of its PN_WAVES hypotheses
struct PnRec {                             // one refinement: the index list idx[idx_off .. idx_off + n_idx) into its problem's points
    int64_t idx_off, word_off;
    int32_t prob, n_idx;
};

struct PnArgs {
    const PnProb *prob;
    const PnBlock *block;
    const SivoPnpPoint *pts;
    const int32_t *samples;    // 4 per hypothesis
    int32_t *count;            // 1 per hypothesis
    double *T;                 // 12 per hypothesis
    uint64_t *bits;            // words per hypothesis
    int lds_cap;
};
struct PnRefArgs {
    const PnProb *prob;
    const PnRec *rec;
    const SivoPnpPoint *pts;
    const int32_t *idx;
    int32_t *count;            // 1 per record
    double *T;                 // 12 per record
    uint64_t *bits;
};

// CheckInliers over all n correspondences of the problem: the first n_lds from the LDS copy, the rest from memory (two loops: one
// load path each).  `live` is uniform in the wave.
__device__ __forceinline__ void pn_check(const double *R, const double *t, const double (&K)[4], const SivoPnpPoint *pts, int n,
                                         const float *lds, int cap, int n_lds, int lane, bool live, uint64_t *bits, int32_t *count_out,
                                         double *T_out) {
    double Rr[9], tr[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rr[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tr[i] = t[i];
    if (!live) return;
    int count = 0;
    for (int base = 0; base < n_lds; base += 64) {
        const int p = base + lane;
        bool in = false;
        if (p < n_lds) {
            const float *s = lds + p;
            in = pnp_inlier(Rr, tr, K, s[0], s[cap], s[2 * cap], s[3 * cap], s[4 * cap], s[5 * cap]);
        }
        const uint64_t word = __ballot(in);
        if (lane == 0) bits[base >> 6] = word;
        count += __popcll(word);
    }
    for (int base = n_lds; base < n; base += 64) {
        const int p = base + lane;
        bool in = false;
        if (p < n) {
            const SivoPnpPoint q = pts[p];
            in = pnp_inlier(Rr, tr, K, q.xw[0], q.xw[1], q.xw[2], q.u, q.v, q.max_err);
        }
        const uint64_t word = __ballot(in);
        if (lane == 0) bits[base >> 6] = word;
        count += __popcll(word);
    }
    if (lane == 0) {
        *count_out = count;
        // (sign and payload of a NaN depend on the machine that produced it: every NaN is stored as the quiet NaN 0x7FF8000000000000)
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const double v = i < 9 ? Rr[i] : tr[i - 9];
            T_out[i] = v != v ? __longlong_as_double(0x7FF8000000000000ll) : v;
        }
    }
}

__global__ __launch_bounds__(PN_THREADS) void pnp_hyp_kernel(PnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float pn_lds[];             // [PN_REC][cap]
    __shared__ PnpWork work[PN_WAVES];
    const int cap = a.lds_cap;
    const PnBlock blk = a.block[blockIdx.x];
    const PnProb &pr = a.prob[blk.prob];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = pr.n;
    const SivoPnpPoint *const pts = a.pts + pr.pt_off;
    const double K[4] = {(double)pr.K[0], (double)pr.K[1], (double)pr.K[2], (double)pr.K[3]};
    for (int p = tid; p < n && p < cap; p += PN_THREADS) {
        const SivoPnpPoint q = pts[p];
        float *s = pn_lds + p;
        s[0] = q.xw[0]; s[cap] = q.xw[1]; s[2 * cap] = q.xw[2]; s[3 * cap] = q.u; s[4 * cap] = q.v; s[5 * cap] = q.max_err;
    }
    __syncthreads();
    int hl = blk.first + wave;                                      // the wave's hypothesis within the problem
    const bool live = hl < pr.n_hyp;
    if (!live) hl = pr.n_hyp - 1;
    const int64_t hg = pr.hyp_off + hl;
    PnpWork &w = work[wave];
    const PnpWaveTeam team{lane};
    const int sol = pnp_epnp(team, w, pts, a.samples + 4 * hg, 4, K);   // (indices checked by the host: 0 <= index < n)
    pn_check(w.Rs[sol], w.ts[sol], K, pts, n, pn_lds, cap, n < cap ? n : cap, lane, live, a.bits + pr.word_off + (int64_t)hl * pr.words,
             a.count + hg, a.T + 12 * hg);
}

__global__ __launch_bounds__(64) void pnp_refine_kernel(PnRefArgs a) {
    __shared__ PnpWork w;
    const PnRec rc = a.rec[blockIdx.x];
    const PnProb &pr = a.prob[rc.prob];
    const int lane = threadIdx.x;
    const SivoPnpPoint *const pts = a.pts + pr.pt_off;
    const double K[4] = {(double)pr.K[0], (double)pr.K[1], (double)pr.K[2], (double)pr.K[3]};
    const PnpWaveTeam team{lane};
    const int sol = pnp_epnp(team, w, pts, a.idx + rc.idx_off, rc.n_idx, K);
    pn_check(w.Rs[sol], w.ts[sol], K, pts, pr.n, nullptr, 0, 0, lane, true, a.bits + rc.word_off, a.count + blockIdx.x, a.T + 12 * (int64_t)blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// Rcw.convertTo(Rcw, CV_32F) (:234-237, :304-307)
static void pn_store_T(float *dst, const double *src) {
    for (int i = 0; i < 12; ++i) {
        float f = (float)src[i];
        if (f != f) { const uint32_t q = 0x7FC00000u; std::memcpy(&f, &q, 4); }
        dst[i] = f;
    }
}

static int pnp_run(SivoPnpRansacProblem *probs, int k) {
    if (k < 0 || k > (1 << 16)) throw std::invalid_argument("problem count out of range");
    if (k > 0 && !probs) throw std::invalid_argument("null argument");
    int64_t points = 0, hyps = 0, words = 0, blocks = 0;
    int max_n = 0;
    for (int i = 0; i < k; ++i) {
        const SivoPnpRansacProblem &p = probs[i];
        if (p.n < 0 || p.n > (1 << 22)) throw std::invalid_argument("point count out of range");
        if (p.n_hyp < 0 || p.n_hyp > (1 << 20)) throw std::invalid_argument("hypothesis count out of range");
        if (p.n && !p.points) throw std::invalid_argument("null argument");
        if (p.n_hyp) {
            if (p.n < 4) throw std::invalid_argument("a hypothesis needs four correspondences");
            if (p.min_inliers < 4) throw std::invalid_argument("min_inliers below the sample size");
            if (!p.samples || !p.count || !p.T || !p.inlier_bits || !p.refined || !p.refined_T || !p.refined_bits)
                throw std::invalid_argument("null argument");
            for (int64_t h = 0; h < p.n_hyp; ++h) {
                const int32_t *s = p.samples + 4 * h;
                for (int a = 0; a < 4; ++a) {
                    if (s[a] < 0 || s[a] >= p.n) throw std::invalid_argument("sample index out of range");
                    for (int b = 0; b < a; ++b)
                        if (s[a] == s[b]) throw std::invalid_argument("a sample repeats an index");
                }
            }
            points += p.n; hyps += p.n_hyp; words += (int64_t)p.n_hyp * cdiv(p.n, 64); blocks += cdiv(p.n_hyp, PN_WAVES);
            max_n = std::max(max_n, p.n);
        }
    }
    if (points > (int64_t)1 << 26 || hyps > (int64_t)1 << 22 || words > (int64_t)1 << 27) throw std::invalid_argument("batch too large");
    for (int i = 0; i < k; ++i) probs[i].n_records = 0;
    if (hyps == 0) return SIVO_OK;
    require_device();
    // the tracking thread evaluates its candidates: pinned staging and device buffers kept per thread, one set per launch (the second
    // launch reads the points the first one uploaded)
    static thread_local SolverCtx c(true, 256 << 10, 0, 256 << 10), c2(true, 64 << 10, 0, 64 << 10);
    c.bind();
    // launch 1.  upload: the problem headers, the workgroup table, then every problem's points and samples back to back (staged in
    // place); results: count, T, inlier words per hypothesis.  One copy each way, one launch, one synchronisation.
    PnArgs a;
    Layout L;
    L.copy(a.prob, nullptr, sizeof(PnProb) * (size_t)k);
    L.copy(a.block, nullptr, sizeof(PnBlock) * (size_t)blocks);
    L.copy(a.pts, nullptr, sizeof(SivoPnpPoint) * (size_t)points);
    L.copy(a.samples, nullptr, 16 * (size_t)hyps);
    L.take(a.count, 4 * (size_t)hyps); L.take(a.T, 96 * (size_t)hyps); L.take(a.bits, 8 * (size_t)words);
    L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
    PnProb *hp = L.host(a.prob);
    PnBlock *hb = L.host(a.block);
    SivoPnpPoint *hpt = L.host(a.pts);
    int32_t *hs = L.host(a.samples);
    int64_t po = 0, ho = 0, wo = 0, bo = 0;
    for (int i = 0; i < k; ++i) {
        const SivoPnpRansacProblem &p = probs[i];
        PnProb &q = hp[i];
        std::memcpy(q.K, p.K, sizeof q.K);
        q.pt_off = po; q.hyp_off = ho; q.word_off = wo;
        q.n = p.n; q.n_hyp = p.n_hyp; q.words = cdiv(p.n, 64); q.pad_ = 0;
        if (!p.n_hyp) continue;
        std::memcpy(hpt + po, p.points, sizeof(SivoPnpPoint) * (size_t)p.n);
        std::memcpy(hs + 4 * ho, p.samples, 16 * (size_t)p.n_hyp);
        for (int f = 0; f < p.n_hyp; f += PN_WAVES) hb[bo++] = PnBlock{i, f};
        po += p.n; ho += p.n_hyp; wo += (int64_t)p.n_hyp * q.words;
    }
    a.lds_cap = std::max(1, std::min(max_n, PN_CAP));
    L.send(c.stream);
    hipLaunchKernelGGL(pnp_hyp_kernel, dim3((unsigned)blocks), dim3(PN_THREADS), pn_lds_bytes(a.lds_cap), c.stream, a);
    SIVO_HIP(hipGetLastError());
    SIVO_HIP(hipMemcpyAsync(L.host(a.count), a.count, L.results(), hipMemcpyDeviceToHost, c.stream));
    SIVO_HIP(hipStreamSynchronize(c.stream));
    const int32_t *cnt = L.host(a.count);
    const double *T = L.host(a.T);
    const uint64_t *bits = L.host(a.bits);
    // iterate() (:228-241) over the counts: a record has count >= min_inliers and count > mnBestInliers
    int64_t recs = 0, idxs = 0, rwords = 0;
    for (int i = 0; i < k; ++i) {
        SivoPnpRansacProblem &p = probs[i];
        if (!p.n_hyp) continue;
        const PnProb &q = hp[i];
        std::memcpy(p.count, cnt + q.hyp_off, 4 * (size_t)p.n_hyp);
        std::memcpy(p.inlier_bits, bits + q.word_off, 8 * (size_t)p.n_hyp * (size_t)q.words);
        int best = p.best_in;
        for (int h = 0; h < p.n_hyp; ++h) {
            pn_store_T(p.T + 12 * (size_t)h, T + 12 * (q.hyp_off + h));
            p.refined[h] = -1;
            if (p.count[h] >= p.min_inliers && p.count[h] > best) {
                best = p.count[h];
                p.refined[h] = 0;
                ++p.n_records; ++recs; idxs += p.count[h]; rwords += q.words;
            }
        }
    }
    if (recs == 0) return SIVO_OK;
    // launch 2: every record of every problem, one workgroup each.  upload: the record table and the index lists (the inliers of each
    // record, ascending: Refine's vIndices, :272-279); results: count, T, inlier words per record.
    c2.bind();
    PnRefArgs r;
    Layout M;
    r.prob = a.prob; r.pts = a.pts;
    M.copy(r.rec, nullptr, sizeof(PnRec) * (size_t)recs);
    M.copy(r.idx, nullptr, 4 * (size_t)idxs);
    M.take(r.count, 4 * (size_t)recs); M.take(r.T, 96 * (size_t)recs); M.take(r.bits, 8 * (size_t)rwords);
    M.place(c2.dev.reserve(M.bytes()), c2.in.reserve(M.bytes()));
    PnRec *hr = M.host(r.rec);
    int32_t *hi = M.host(r.idx);
    int64_t ro = 0, io = 0, rw = 0;
    for (int i = 0; i < k; ++i) {
        const SivoPnpRansacProblem &p = probs[i];
        if (!p.n_records) continue;
        const PnProb &q = hp[i];
        for (int h = 0; h < p.n_hyp; ++h) {
            if (p.refined[h] < 0) continue;
            hr[ro++] = PnRec{io, rw, i, p.count[h]};
            const uint64_t *b = p.inlier_bits + (size_t)h * q.words;
            for (int j = 0; j < p.n; ++j)
                if (b[j >> 6] >> (j & 63) & 1) hi[io++] = j;
            rw += q.words;
        }
    }
    M.send(c2.stream);
    hipLaunchKernelGGL(pnp_refine_kernel, dim3((unsigned)recs), dim3(64), 0, c2.stream, r);
    SIVO_HIP(hipGetLastError());
    SIVO_HIP(hipMemcpyAsync(M.host(r.count), r.count, M.results(), hipMemcpyDeviceToHost, c2.stream));
    SIVO_HIP(hipStreamSynchronize(c2.stream));
    const int32_t *rcnt = M.host(r.count);
    const double *rT = M.host(r.T);
    const uint64_t *rbits = M.host(r.bits);
    ro = 0; rw = 0;
    for (int i = 0; i < k; ++i) {
        SivoPnpRansacProblem &p = probs[i];
        if (!p.n_records) continue;
        const PnProb &q = hp[i];
        for (int h = 0; h < p.n_hyp; ++h) {
            if (p.refined[h] < 0) continue;
            p.refined[h] = rcnt[ro];
            pn_store_T(p.refined_T + 12 * (size_t)h, rT + 12 * ro);
            std::memcpy(p.refined_bits + (size_t)h * q.words, rbits + rw, 8 * (size_t)q.words);
            ++ro; rw += q.words;
        }
    }
    return SIVO_OK;
}

}  // namespace sivo

using namespace sivo;

extern "C" int sivo_pnp_ransac_batch(SivoPnpRansacProblem *problems, int n_problems) {
    return guarded([&] { return pnp_run(problems, n_problems); });
}

extern "C" int sivo_pnp_ransac(SivoPnpRansacProblem *problem) {
    return guarded([&] {
        if (!problem) throw std::invalid_argument("null argument");
        return pnp_run(problem, 1);
    });
}
