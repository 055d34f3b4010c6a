// fuse_batch.hip — ORBmatcher::Fuse of one list of map points into EVERY target keyframe in one launch: the loops of
// LocalMapping::SearchInNeighbors (reference src/orbslam/LocalMapping.cc:586-594) and LoopClosing::SearchAndFuse (LoopClosing.cc:609-635)
// up to the choice of the keypoint (ORBmatcher.cc:814-909 / :966-1036).
//
// One wave per (keyframe, point) pair, four pairs per workgroup, as search_round_kernel (search.hip): the wave runs the per-point tests
// of fuse_math.hpp (every lane the same arithmetic: the pair is wave-uniform), then walks the keyframe's grid cells as that kernel's
// window branch does — the cells a window covers are contiguous per grid column in the frame's CSR, the 64 lanes stride the candidates —
// applies the octave test and, in the Tcw form, the chi-square gates, takes the Hamming distance and merges the lanes' best on a
// (distance, visiting order) key, which is the reference's first-minimum-wins scan over GetFeaturesInArea's order.  Fuse has no
// dependence between queries (which key a point would fuse with does not depend on the surgery of the others), so there are no rounds:
// one staged copy up (the keyframes' view table and cameras, the points, the masks), one launch, one copy down.
//
// The keyframes are sivo_mframe handles: the kernel reads their slabs through a table of pointers.  Each frame owns a stream on which
// its upload may still be in flight; the call waits for each of them before it launches on the stream of its own, and returns only when
// its kernel has finished, so the frames serve sivo_fuse / sivo_search again as before.  The staging buffers are grow-only and kept per
// device: a call allocates nothing once a call of its size has run.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.hpp"
#include "fuse_math.hpp"
#include "mframe.hpp"
#include "solver_host.hpp"

namespace sivo {
namespace {

struct FuseKfView {                // what the kernel reads of one sivo_mframe (pointers into its slab)
    const float *x, *y, *ur, *scale, *inv_sigma2;      // ur: null for a frame without mvRight
    const int32_t *oct, *cell_off, *cell_idx;
    const uint4 *desc;
    float min_x, min_y, inv_w, inv_h;
    int32_t n, pad_;
};

struct FuseBatchArgs {
    const FuseKfView *views;
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

constexpr uint32_t FU_KEY_NONE = 0xffffffffu;

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
    const FuseKfView V = a.views[k];
    const float radius = a.th * V.scale[o.level];                  // :852 (the camera's nlevels is not above the frame's)
    const int lvl_lo = o.level - 1, lvl_hi = o.level;
    const bool gates = cam.c.scw_variant == 0;
    const uint4 q0 = a.desc[(int64_t)i * 2], q1 = a.desc[(int64_t)i * 2 + 1];
    uint32_t key = FU_KEY_NONE;
    int idx1 = -1, seen = 0;
    // window -> cell ranges, exactly as Frame::GetFeaturesInArea (Frame.cc:334-357)
    const int cx0 = max(0, (int)floorf((o.u - V.min_x - radius) * V.inv_w));
    const int cx1 = min(SIVO_GRID_COLS - 1, (int)ceilf((o.u - V.min_x + radius) * V.inv_w));
    const int cy0 = max(0, (int)floorf((o.v - V.min_y - radius) * V.inv_h));
    const int cy1 = min(SIVO_GRID_ROWS - 1, (int)ceilf((o.v - V.min_y + radius) * V.inv_h));
    if (cx0 < SIVO_GRID_COLS && cx1 >= 0 && cy0 < SIVO_GRID_ROWS && cy1 >= 0) {
        uint32_t base = 0;
        for (int ix = cx0; ix <= cx1; ++ix) {
            const int s = V.cell_off[ix * SIVO_GRID_ROWS + cy0], e = V.cell_off[ix * SIVO_GRID_ROWS + cy1 + 1];
            for (int j = s + lane; j < e; j += 64) {
                const int idx = V.cell_idx[j];
                const float kx = V.x[idx], ky = V.y[idx];
                if (!(fabsf(kx - o.u) < radius && fabsf(ky - o.v) < radius)) continue;       // Frame.cc:379-384
                seen = 1;                                                                    // vIndices is not empty (:856)
                const int lvl = V.oct[idx];
                if (lvl < lvl_lo || lvl > lvl_hi) continue;                                  // :875
                if (gates) {                                                                 // :878-899
                    const float kur = V.ur ? V.ur[idx] : -1.0f;
                    const float ex = o.u - kx, ey = o.v - ky;
                    if (kur >= 0) {
                        const float er = o.ur - kur;
                        const float e2 = ex * ex + ey * ey + er * er;
                        if ((double)(e2 * V.inv_sigma2[lvl]) > 7.8) continue;
                    } else {
                        const float e2 = ex * ex + ey * ey;
                        if ((double)(e2 * V.inv_sigma2[lvl]) > 5.99) continue;
                    }
                }
                const int d = ham256(q0, q1, V.desc[(int64_t)idx * 2], V.desc[(int64_t)idx * 2 + 1]);
                if (d >= 256) continue;                  // `dist < bestDist` from 256; from INT_MAX a 256 would be taken and then fail TH_LOW
                const uint32_t kk = ((uint32_t)d << 22) | (base + (uint32_t)(j - s));
                if (kk < key) { key = kk; idx1 = idx; }
            }
            base += (uint32_t)(e - s);
        }
    }
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

// The call's state on one device: a stream of its own and the grow-only staging buffers (pinned mirror and device block of one layout).
struct FuseCtx {
    std::mutex mu;
    hipStream_t stream = nullptr;
    PinnedBuf host{1 << 20};
    DeviceBuf dev{1 << 20};
};
FuseCtx &fuse_ctx(int device) {                // (with the device current) never destroyed: a call may come after main() returns
    static std::mutex mu;
    static FuseCtx *ctx[64] = {};
    std::lock_guard<std::mutex> lock(mu);
    if (device < 0 || device >= 64) throw std::runtime_error("sivo_fuse_batch: device index outside 0 .. 63");
    if (!ctx[device]) {
        FuseCtx *c = new FuseCtx;
        SIVO_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        ctx[device] = c;
    }
    return *ctx[device];
}

size_t al(size_t bytes) { return (bytes + 255) / 256 * 256; }
template <class T>
T *carve(char *&p, size_t count) {
    T *r = reinterpret_cast<T *>(p);
    p += al(count * sizeof(T));
    return r;
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
        const int device = kfs[0]->device;
        DeviceGuard dg(device);
        FuseCtx &c = fuse_ctx(device);
        std::lock_guard<std::mutex> lock(c.mu);
        const size_t K = (size_t)n_kf, N = (size_t)n_mp, KN = K * N;
        const bool extras = u || v || ur || level;
        // [ upload | download ], the pinned mirror in the same layout
        const size_t up_bytes = al(K * sizeof(FuseKfView)) + al(K * sizeof(FuCamera)) + 2 * al(12 * N) + 2 * al(4 * N) + al(32 * N) + al(N) + al(KN);
        const size_t down_bytes = 2 * al(4 * KN) + al(KN) + (extras ? 4 * al(4 * KN) : 0);
        char *const d0 = c.dev.reserve(up_bytes + down_bytes);
        char *const h0 = c.host.reserve(up_bytes + down_bytes);
        auto host = [&](auto *dev) { return reinterpret_cast<decltype(dev)>(h0 + ((char *)dev - d0)); };
        char *p = d0;
        FuseBatchArgs a{};
        FuseKfView *d_views = carve<FuseKfView>(p, K);
        FuCamera *d_cams = carve<FuCamera>(p, K);
        float *d_pos = carve<float>(p, 3 * N), *d_normal = carve<float>(p, 3 * N), *d_min = carve<float>(p, N), *d_max = carve<float>(p, N);
        uint4 *d_desc = carve<uint4>(p, 2 * N);
        uint8_t *d_skip_point = carve<uint8_t>(p, N), *d_skip_pair = carve<uint8_t>(p, KN);
        char *const down0 = p;
        a.best_idx = carve<int32_t>(p, KN); a.best_dist = carve<int32_t>(p, KN); a.status = carve<uint8_t>(p, KN);
        if (extras) { a.u = carve<float>(p, KN); a.v = carve<float>(p, KN); a.ur = carve<float>(p, KN); a.level = carve<int32_t>(p, KN); }
        // each frame's own upload runs on the frame's stream: it must have landed before the kernel reads the slab
        for (size_t k = 0; k < K; ++k) SIVO_HIP(hipStreamSynchronize(kfs[k]->stream));
        FuseKfView *hv = host(d_views);
        FuCamera *hc = host(d_cams);
        for (size_t k = 0; k < K; ++k) {
            const sivo_mframe &F = *kfs[k];
            FuseKfView &V = hv[k];
            V.x = F.d_x; V.y = F.d_y; V.ur = F.u_right.empty() ? nullptr : F.d_ur; V.scale = F.d_scale; V.inv_sigma2 = F.d_inv_sigma2;
            V.oct = F.d_oct; V.cell_off = F.d_cell_off; V.cell_idx = F.d_cell_idx; V.desc = F.d_desc;
            V.min_x = F.min_x; V.min_y = F.min_y; V.inv_w = F.inv_w; V.inv_h = F.inv_h; V.n = F.n; V.pad_ = 0;
            fu_camera(cams[k], hc[k]);
        }
        std::memcpy(host(d_pos), pos, 12 * N);
        std::memcpy(host(d_normal), normal, 12 * N);
        std::memcpy(host(d_min), min_dist, 4 * N);
        std::memcpy(host(d_max), max_dist, 4 * N);
        std::memcpy(host(d_desc), mp_desc, 32 * N);
        if (skip_point) std::memcpy(host(d_skip_point), skip_point, N);
        if (skip_pair) std::memcpy(host(d_skip_pair), skip_pair, KN);
        SIVO_HIP(hipMemcpyAsync(d0, h0, up_bytes, hipMemcpyHostToDevice, c.stream));
        a.views = d_views; a.cams = d_cams; a.n_kf = n_kf; a.n_mp = n_mp;
        a.pos = d_pos; a.normal = d_normal; a.min_dist = d_min; a.max_dist = d_max; a.desc = d_desc;
        a.skip_point = skip_point ? d_skip_point : nullptr; a.skip_pair = skip_pair ? d_skip_pair : nullptr;
        a.th = th;
        hipLaunchKernelGGL(fuse_batch_kernel, dim3((unsigned)cdiv64((int64_t)KN, 4)), dim3(256), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipMemcpyAsync(h0 + (down0 - d0), down0, down_bytes, hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        std::memcpy(best_idx, host(a.best_idx), 4 * KN);
        std::memcpy(best_dist, host(a.best_dist), 4 * KN);
        const uint8_t *hs = host(a.status);
        std::memcpy(status, hs, KN);
        if (extras) {
            const float *hu = host(a.u), *hvv = host(a.v), *hr = host(a.ur);
            const int32_t *hl = host(a.level);
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
