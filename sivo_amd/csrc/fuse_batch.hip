// fuse_batch.hip — ORBmatcher::Fuse of one list of map points into EVERY target keyframe in one launch: the loops of
// LocalMapping::SearchInNeighbors (reference src/orbslam/LocalMapping.cc:586-594) and LoopClosing::SearchAndFuse (LoopClosing.cc:609-635)
// up to the choice of the keypoint (ORBmatcher.cc:814-909 / :966-1036).
//
// One wave per (keyframe, point) pair, four pairs per workgroup, as search_round_kernel (search.hip): the wave runs the per-point tests
// of fuse_math.hpp (every lane the same arithmetic: the pair is wave-uniform), then walks the keyframe's grid with the scan_window that
// kernel's window branch uses (mframe.hpp), applies the octave test and, in the Tcw form, the chi-square gate (grid_math.hpp), takes the
// Hamming distance and merges the lanes' best on match_key's (distance, visiting order), which is the reference's first-minimum-wins
// scan over GetFeaturesInArea's order.  Fuse has no dependence between queries (which key a point would fuse with does not depend on the
// surgery of the others), so there are no rounds: one staged copy up (the keyframes' views and cameras, the points, the masks), one
// launch, one copy down.
//
// The keyframes are sivo_mframe handles: the kernel reads their slabs through a table of MframeView.  Each frame owns a stream on which
// its upload may still be in flight; the call waits for each of them before it launches on the stream of its own, and returns only when
// its kernel has finished, so the frames serve sivo_fuse / sivo_search again as before.  Staging is the library's usual one: a SolverCtx
// per calling thread (stream, grow-only buffers) and one Layout per call (solver_host.hpp); a call allocates nothing once a call of its
// size has run on the thread.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <cstring>
#include <stdexcept>
#include <string>

#include "common.hpp"
#include "fuse_math.hpp"
#include "mframe.hpp"
#include "solver_host.hpp"

namespace sivo {
namespace {

struct FuseBatchArgs {
    const MframeView *views;
    const FuCamera *cams;
    int n_kf, n_mp;
    const float *pos, *normal, *min_dist, *max_dist;
    const uint4 *desc;
    const uint8_t *skip_point, *skip_pair;             // each may be null
    float th;
    int32_t *best_idx, *best_dist;
    uint8_t *status;
    float *u, *v, *ur;                                 // null when the caller asked for none of the four
    int32_t *level;
};

__global__ __launch_bounds__(256) void fuse_batch_kernel(FuseBatchArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (int64_t)a.n_kf * a.n_mp) return;
    const int k = (int)(pair / a.n_mp), i = (int)(pair - (int64_t)k * a.n_mp);
    const FuCamera &cam = a.cams[k];
    const int none_dist = cam.c.scw_variant ? INT_MAX : 256;       // bestDist as the loop leaves it without a comparison (:863 / :1017)
    uint8_t st = SIVO_FUSE_SKIPPED;
    FuResult o;
    if (!(a.skip_point && a.skip_point[i]) && !(a.skip_pair && a.skip_pair[pair])) {
        const float X[3] = {a.pos[3 * (int64_t)i], a.pos[3 * (int64_t)i + 1], a.pos[3 * (int64_t)i + 2]};
        const float N[3] = {a.normal[3 * (int64_t)i], a.normal[3 * (int64_t)i + 1], a.normal[3 * (int64_t)i + 2]};
        st = fu_point(cam, X, N, a.min_dist[i], a.max_dist[i], o);
    }
    if (st != SIVO_FUSE_REACHED) {
        if (lane == 0) { a.best_idx[pair] = -1; a.best_dist[pair] = none_dist; a.status[pair] = st; }
        return;
    }
    const MframeView V = a.views[k];
    const float radius = a.th * V.scale[o.level];                  // :852 (the camera's nlevels is not above the frame's)
    const int lvl_lo = o.level - 1, lvl_hi = o.level;
    const bool gates = cam.c.scw_variant == 0;
    const uint4 q0 = a.desc[(int64_t)i * 2], q1 = a.desc[(int64_t)i * 2 + 1];
    uint32_t key = KEY_NONE;
    int idx1 = -1, seen = 0;
    scan_window(V, o.u, o.v, radius, lane, [&](int idx, uint32_t ord) {
        const float kx = V.x[idx], ky = V.y[idx];
        if (!in_window(kx, ky, o.u, o.v, radius)) return;
        seen = 1;                                                  // vIndices is not empty (:856)
        const int lvl = V.oct[idx];
        if (lvl < lvl_lo || lvl > lvl_hi) return;                  // :875
        if (gates) {
            const float kur = V.ur ? V.ur[idx] : -1.0f;
            if (!fuse_chi2_gate(o.u - kx, o.v - ky, kur >= 0, o.ur - kur, V.inv_sigma2[lvl])) return;
        }
        const int d = ham256(q0, q1, V.desc[(int64_t)idx * 2], V.desc[(int64_t)idx * 2 + 1]);
        if (d >= 256) return;                // `dist < bestDist` from 256; from INT_MAX a 256 would be taken and then fail TH_LOW
        const uint32_t kk = match_key(d, ord);
        if (kk < key) { key = kk; idx1 = idx; }
    });
    // butterfly: the smallest (distance, visiting order) of the wave
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t ok = __shfl_xor(key, off);
        const int oi = __shfl_xor(idx1, off);
        seen |= __shfl_xor(seen, off);
        if (ok < key) { key = ok; idx1 = oi; }
    }
    if (lane != 0) return;
    const int best = idx1 >= 0 ? (int)(key >> 22) : none_dist;
    const bool accept = idx1 >= 0 && best <= SIVO_TH_LOW;          // :912
    a.best_idx[pair] = accept ? idx1 : -1;
    a.best_dist[pair] = best;
    a.status[pair] = accept ? SIVO_FUSE_MATCHED : seen ? SIVO_FUSE_TOO_FAR : SIVO_FUSE_NO_CANDIDATE;
    if (a.u) { a.u[pair] = o.u; a.v[pair] = o.v; a.ur[pair] = o.ur; a.level[pair] = o.level; }
}

SolverCtx &fb_ctx() {
    static thread_local SolverCtx c(false, 1 << 20, 0, 1 << 20);
    c.bind();
    return c;
}

}  // namespace
}  // namespace sivo

using namespace sivo;

extern "C" int sivo_fuse_batch(const sivo_mframe_t *kfs, const SivoFuseCamera *cams, int n_kf, int n_mp, const float *pos,
                               const float *normal, const float *min_dist, const float *max_dist, const uint8_t *mp_desc,
                               const uint8_t *skip_point, const uint8_t *skip_pair, float th, int32_t *best_idx, int32_t *best_dist,
                               uint8_t *status, float *u, float *v, float *ur, int32_t *level) {
    return guarded([&] {
        if (const char *e = fu_check_batch(kfs, cams, n_kf, n_mp, pos, normal, min_dist, max_dist, mp_desc, best_idx, best_dist, status))
            throw std::invalid_argument(std::string("sivo_fuse_batch: ") + e);
        if (n_kf == 0 || n_mp == 0) return SIVO_OK;
        for (int k = 0; k < n_kf; ++k)
            if (kfs[k]->n >= (1 << 22)) throw std::invalid_argument("sivo_fuse_batch: at most 2^22 - 1 keypoints per frame");
        require_device();
        DeviceGuard dg(kfs[0]->device);
        SolverCtx &c = fb_ctx();
        const size_t K = (size_t)n_kf, N = (size_t)n_mp, KN = K * N;
        const bool extras = u || v || ur || level;
        FuseBatchArgs a{};
        Layout L;
        L.copy(a.views, nullptr, K * sizeof(MframeView)); L.copy(a.cams, nullptr, K * sizeof(FuCamera));      // written below
        L.copy(a.pos, pos, 12 * N); L.copy(a.normal, normal, 12 * N); L.copy(a.min_dist, min_dist, 4 * N); L.copy(a.max_dist, max_dist, 4 * N);
        L.copy(a.desc, mp_desc, 32 * N);
        if (skip_point) L.copy(a.skip_point, skip_point, N);
        if (skip_pair) L.copy(a.skip_pair, skip_pair, KN);
        L.take(a.best_idx, 4 * KN); L.take(a.best_dist, 4 * KN); L.take(a.status, KN);
        if (extras) { L.take(a.u, 4 * KN); L.take(a.v, 4 * KN); L.take(a.ur, 4 * KN); L.take(a.level, 4 * KN); }
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        a.n_kf = n_kf; a.n_mp = n_mp; a.th = th;
        // each frame's own upload runs on the frame's stream: it must have landed before the kernel reads the slab
        for (size_t k = 0; k < K; ++k) SIVO_HIP(hipStreamSynchronize(kfs[k]->stream));
        MframeView *hv = L.host(a.views);
        FuCamera *hc = L.host(a.cams);
        for (size_t k = 0; k < K; ++k) {
            hv[k] = kfs[k]->view();
            fu_camera(cams[k], hc[k]);
        }
        L.send(c.stream);
        hipLaunchKernelGGL(fuse_batch_kernel, dim3((unsigned)cdiv64((int64_t)KN, 4)), dim3(256), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipMemcpyAsync(L.host(a.best_idx), a.best_idx, L.results(), hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        std::memcpy(best_idx, L.host(a.best_idx), 4 * KN);
        std::memcpy(best_dist, L.host(a.best_dist), 4 * KN);
        const uint8_t *hs = L.host(a.status);
        std::memcpy(status, hs, KN);
        if (extras) {
            const float *hu = L.host(a.u), *hvv = L.host(a.v), *hr = L.host(a.ur);
            const int32_t *hl = L.host(a.level);
            for (size_t j = 0; j < KN; ++j) {
                if (hs[j] != SIVO_FUSE_MATCHED && hs[j] != SIVO_FUSE_NO_CANDIDATE && hs[j] != SIVO_FUSE_TOO_FAR) continue;   // left alone
                if (u) u[j] = hu[j];
                if (v) v[j] = hvv[j];
                if (ur) ur[j] = hr[j];
                if (level) level[j] = hl[j];
            }
        }
        return SIVO_OK;
    });
}
