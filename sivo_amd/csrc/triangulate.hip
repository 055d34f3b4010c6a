// triangulate.hip — the loop over the matches of LocalMapping::CreateNewMapPoints (reference src/orbslam/LocalMapping.cc:277-470), the step
// of LocalMapping::Run between SearchForTriangulation and the new MapPoints: parallax test, linear triangulation or stereo unprojection,
// depth, reprojection and scale-consistency tests and both CheckSemantics calls, for every match of a keyframe pair at once.  Every
// match is independent of every other: one thread per match, workgroups of one wave; a batch of pairs is one launch through a workgroup
// table (the single call is the batch of one: the same kernel, the same bytes).  The keyframe headers are read through the workgroup's
// uniform problem index: scalar loads.  A few hundred matches per call: latency bound, like the RANSAC kernels.
//
// Arithmetic: triangulate_math.hpp, which g++ also compiles for the host; tests/triangulate_restatement.py restates it in numpy and is
// compared bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "common.hpp"
#include "solver_host.hpp"

#pragma clang fp contract(off)

#include "triangulate_math.hpp"

namespace sivo {

constexpr int TR_THREADS = 64;

struct TrProb {                // one keyframe pair as staged on the device
    SivoTriKeyFrame kf1, kf2;
    double Sx[36];
    double th_conf, th_ent;
    int64_t match_off;         // first match of the problem in the batch's arrays
    int32_t n;
    float ratio_factor;
};
struct TrBlock { int32_t prob, first; };   // workgroup -> its problem and the first of its TR_THREADS matches

struct TrArgs {
    const TrProb *prob;
    const TrBlock *block;
    const SivoTriMatch *matches;
    uint32_t *wP;              // 3 per match, the float's bits
    uint8_t *status, *cls;     // 1 per match
};

__global__ __launch_bounds__(TR_THREADS) void triangulate_kernel(TrArgs a) {
    const TrBlock blk = a.block[blockIdx.x];
    const TrProb &pr = a.prob[blk.prob];
    const int i = blk.first + (int)threadIdx.x;
    if (i >= pr.n) return;
    const int64_t g = pr.match_off + i;
    const SivoTriMatch m = a.matches[g];
    TrResult o;
    tr_match(pr.kf1, pr.kf2, pr.ratio_factor, pr.Sx, pr.th_conf, pr.th_ent, m, o);
    a.status[g] = o.status;
    a.cls[g] = o.cls;
    a.wP[3 * g] = tr_float_bits(o.wP[0]); a.wP[3 * g + 1] = tr_float_bits(o.wP[1]); a.wP[3 * g + 2] = tr_float_bits(o.wP[2]);
}

static void tr_check_kf(const SivoTriKeyFrame &k) {
    if (k.nlevels < 1 || k.nlevels > 16) throw std::invalid_argument("nlevels outside 1 .. 16");
}

static int tr_run(SivoTriProblem *probs, int k) {
    if (k < 0 || k > (1 << 16)) throw std::invalid_argument("problem count out of range");
    if (k > 0 && !probs) throw std::invalid_argument("null argument");
    int64_t matches = 0, blocks = 0;
    for (int i = 0; i < k; ++i) {
        const SivoTriProblem &p = probs[i];
        if (p.n < 0 || p.n > (1 << 24)) throw std::invalid_argument("match count out of range");
        tr_check_kf(p.kf1); tr_check_kf(p.kf2);
        if (p.n == 0) continue;
        if (!p.matches || !p.status || !p.wP || !p.detected_class) throw std::invalid_argument("null argument");
        for (int j = 0; j < p.n; ++j) {
            const SivoTriMatch &m = p.matches[j];
            if (m.octave1 < 0 || m.octave1 >= p.kf1.nlevels || m.octave2 < 0 || m.octave2 >= p.kf2.nlevels)
                throw std::invalid_argument("octave out of range");
        }
        matches += p.n; blocks += cdiv(p.n, TR_THREADS);
    }
    if (matches > (int64_t)1 << 26) throw std::invalid_argument("batch too large");
    if (matches == 0) return SIVO_OK;
    require_device();
    // the local mapper triangulates one neighbour after the other: pinned staging and device buffers kept per thread.  Upload: the problem
    // headers, the workgroup table, every problem's matches back to back (staged in place); results: wP, status, class per match.  One
    // copy each way, one launch, one synchronisation.
    static thread_local SolverCtx c(true, 256 << 10, 0, 256 << 10);
    c.bind();
    TrArgs a;
    Layout L;
    L.copy(a.prob, nullptr, sizeof(TrProb) * (size_t)k);
    L.copy(a.block, nullptr, sizeof(TrBlock) * (size_t)blocks);
    L.copy(a.matches, nullptr, sizeof(SivoTriMatch) * (size_t)matches);
    L.take(a.wP, 12 * (size_t)matches); L.take(a.status, (size_t)matches); L.take(a.cls, (size_t)matches);
    L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
    TrProb *hp = L.host(a.prob);
    TrBlock *hb = L.host(a.block);
    SivoTriMatch *hm = L.host(a.matches);
    int64_t mo = 0, bo = 0;
    for (int i = 0; i < k; ++i) {
        const SivoTriProblem &p = probs[i];
        TrProb &q = hp[i];
        q.kf1 = p.kf1; q.kf2 = p.kf2;
        std::memcpy(q.Sx, p.state_cov, sizeof q.Sx);
        q.th_conf = p.th_confidence; q.th_ent = p.th_entropy;
        q.match_off = mo; q.n = p.n; q.ratio_factor = p.ratio_factor;
        if (!p.n) continue;
        std::memcpy(hm + mo, p.matches, sizeof(SivoTriMatch) * (size_t)p.n);
        for (int f = 0; f < p.n; f += TR_THREADS) hb[bo++] = TrBlock{i, f};
        mo += p.n;
    }
    L.send(c.stream);
    hipLaunchKernelGGL(triangulate_kernel, dim3((unsigned)blocks), dim3(TR_THREADS), 0, c.stream, a);
    SIVO_HIP(hipGetLastError());
    SIVO_HIP(hipMemcpyAsync(L.host(a.wP), a.wP, L.results(), hipMemcpyDeviceToHost, c.stream));
    SIVO_HIP(hipStreamSynchronize(c.stream));
    const uint32_t *wP = L.host(a.wP);
    const uint8_t *st = L.host(a.status), *cl = L.host(a.cls);
    for (int i = 0; i < k; ++i) {
        const SivoTriProblem &p = probs[i];
        if (!p.n) continue;
        const int64_t off = hp[i].match_off;
        std::memcpy(p.wP, wP + 3 * off, 12 * (size_t)p.n);
        std::memcpy(p.status, st + off, (size_t)p.n);
        std::memcpy(p.detected_class, cl + off, (size_t)p.n);
    }
    return SIVO_OK;
}

}  // namespace sivo

using namespace sivo;

extern "C" int sivo_triangulate_batch(SivoTriProblem *problems, int n_problems) {
    return guarded([&] { return tr_run(problems, n_problems); });
}

extern "C" int sivo_triangulate(SivoTriProblem *problem) {
    return guarded([&] {
        if (!problem) throw std::invalid_argument("null argument");
        return tr_run(problem, 1);
    });
}
