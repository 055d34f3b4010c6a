// mappoint.hip — MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (reference src/orbslam/MapPoint.cc:284-347,
// :368-411) for a batch of map points: what LocalMapping::ProcessNewKeyFrame (LocalMapping.cc:116-123), CreateNewMapPoints (:461-463),
// SearchInNeighbors (:628-634), the optimizers' write-back and LoopClosing::CorrectLoop run point after point on the host.
//
// One wave per point, one workgroup per wave.  Lane i holds row i of the N x N Hamming matrix: it finds the row's median by rank
// selection (mappoint_math.hpp: nine counting passes over the point's descriptors, which every lane reads at the same address — one
// cache line broadcast), rows i + 64, i + 128, ... of a point with more than 64 descriptors follow in the same loop; the first row with
// the strictly smallest median is the minimum of (median, row) over the wave.  Lane 0 then walks the observations in order for the
// normal: a running float sum whose order is the reference's.  A few thousand points of ten to thirty observations: latency bound.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "common.hpp"
#include "solver_host.hpp"

#pragma clang fp contract(off)

#include "mappoint_math.hpp"

namespace sivo {

struct MpArgs {
    const int64_t *desc_off, *obs_off;     // np + 1 each
    const uint64_t *desc;                  // 4 per descriptor
    const float *obs_ow;                   // 3 per observation
    const float *point;                    // 8 per point: pos[3], ref_ow[3], level_scale, last_scale
    int32_t *best_idx;                     // 1 per point
    uint32_t *geom;                        // 5 per point: max, min, normal[3] (the float's bits)
    uint8_t *flags;
    int np;
};

__global__ __launch_bounds__(64) void mappoint_refresh_kernel(MpArgs a) {
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= a.np) return;
    const int64_t d0 = a.desc_off[p], N = a.desc_off[p + 1] - d0, o0 = a.obs_off[p], M = a.obs_off[p + 1] - o0;
    if (M == 0) {                                                   // (:299-301, :385-387)
        if (lane == 0) a.flags[p] = SIVO_MP_NO_OBSERVATION | SIVO_MP_NO_DESCRIPTOR;
        return;
    }
    if (N > 0) {
        const uint64_t *desc = a.desc + 4 * d0;
        // key = median << 32 | row: its minimum is the first row with the strictly smallest median (:337-340)
        int64_t key = INT64_MAX;
        for (int64_t i = lane; i < N; i += 64) {
            const int64_t k = ((int64_t)mp_row_median(desc, N, i) << 32) | i;
            key = k < key ? k : key;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const int64_t other = __shfl_xor(key, m, 64);
            key = other < key ? other : key;
        }
        if (lane == 0) a.best_idx[p] = (int32_t)(key & 0xFFFFFFFFll);
    }
    if (lane == 0) {
        const float *pt = a.point + 8 * (int64_t)p;
        float out[5];
        mp_normal_depth(pt, a.obs_ow + 3 * o0, M, pt + 3, pt[6], pt[7], out);
#pragma unroll
        for (int i = 0; i < 5; ++i) a.geom[5 * (int64_t)p + i] = out[i] != out[i] ? 0x7FC00000u : __float_as_uint(out[i]);
        a.flags[p] = N > 0 ? 0 : SIVO_MP_NO_DESCRIPTOR;
    }
}

static void mp_check_offsets(const int64_t *off, int np, const char *what) {
    if (off[0] != 0) throw std::invalid_argument(std::string(what) + " offsets do not start at 0");
    for (int p = 0; p < np; ++p)
        if (off[p + 1] < off[p]) throw std::invalid_argument(std::string(what) + " offsets decrease");
    if (off[np] > (int64_t)1 << 26) throw std::invalid_argument(std::string(what) + " count out of range");
    for (int p = 0; p < np; ++p)
        if (off[p + 1] - off[p] > (1 << 20)) throw std::invalid_argument(std::string(what) + ": more than 2^20 in one point");
}

}  // namespace sivo

using namespace sivo;

extern "C" int sivo_mappoint_refresh(int np, const int64_t *desc_off, const uint8_t *desc, const int64_t *obs_off, const float *obs_ow,
                                     const float *pos, const float *ref_ow, const float *level_scale, const float *last_scale,
                                     int32_t *best_idx, float *max_dist, float *min_dist, float *normal, uint8_t *flags) {
    return guarded([&] {
        if (np < 0 || np > (1 << 22)) throw std::invalid_argument("point count out of range");
        if (np == 0) return SIVO_OK;
        if (!desc_off || !obs_off || !pos || !ref_ow || !level_scale || !last_scale || !best_idx || !max_dist || !min_dist || !normal || !flags)
            throw std::invalid_argument("null argument");
        mp_check_offsets(desc_off, np, "descriptor");
        mp_check_offsets(obs_off, np, "observation");
        const size_t nd = (size_t)desc_off[np], no = (size_t)obs_off[np], P = (size_t)np;
        if ((nd && !desc) || (no && !obs_ow)) throw std::invalid_argument("null argument");
        require_device();
        // one staged upload (offsets, descriptors, camera centres, the per-point record), results in one copy back, one synchronisation
        static thread_local SolverCtx c(true, 1 << 20, 0, 1 << 20);
        c.bind();
        MpArgs a;
        Layout L;
        L.copy(a.desc_off, desc_off, 8 * (P + 1)); L.copy(a.obs_off, obs_off, 8 * (P + 1));
        L.copy(a.desc, desc, 32 * nd); L.copy(a.obs_ow, obs_ow, 12 * no);
        L.copy(a.point, nullptr, 32 * P);
        L.take(a.best_idx, 4 * P); L.take(a.geom, 20 * P); L.take(a.flags, P);
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        float *hp = L.host(a.point);
        for (size_t p = 0; p < P; ++p) {
            float *q = hp + 8 * p;
            std::memcpy(q, pos + 3 * p, 12); std::memcpy(q + 3, ref_ow + 3 * p, 12);
            q[6] = level_scale[p]; q[7] = last_scale[p];
        }
        a.np = np;
        L.send(c.stream);
        hipLaunchKernelGGL(mappoint_refresh_kernel, dim3((unsigned)np), dim3(64), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipMemcpyAsync(L.host(a.best_idx), a.best_idx, L.results(), hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        const int32_t *hb = L.host(a.best_idx);
        const uint32_t *hg = L.host(a.geom);
        const uint8_t *hf = L.host(a.flags);
        for (size_t p = 0; p < P; ++p) {
            flags[p] = hf[p];
            if (hf[p] & SIVO_MP_NO_OBSERVATION) continue;            // nothing of the point is written
            if (!(hf[p] & SIVO_MP_NO_DESCRIPTOR)) best_idx[p] = hb[p];
            std::memcpy(max_dist + p, hg + 5 * p, 4); std::memcpy(min_dist + p, hg + 5 * p + 1, 4);
            std::memcpy(normal + 3 * p, hg + 5 * p + 2, 12);
        }
        return SIVO_OK;
    });
}
