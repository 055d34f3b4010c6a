// covis.hip — the covisibility bookkeeping of the three SLAM threads on arrays: the counting loop of KeyFrame::UpdateConnections (reference
// src/orbslam/KeyFrame.cc:340-360) and of Tracking::UpdateLocalKeyFrames (Tracking.cc:1129-1142), the whole of
// LocalMapping::KeyFrameCulling (LocalMapping.cc:732-791) and the branches of LocalMapping::MapPointCulling (LocalMapping.cc:181-194).
// The reference copies a std::map per point (GetObservations() returns by value); here the observation lists are one CSR table.
//
// covis_count_kernel: one workgroup per slot list.  The histogram over keyframes lives in LDS (integer atomics, cleared and written out
// in strides); above SIVO_COVIS_LDS_KF keyframes the adds go to the zeroed output row in global memory.  Integer adds: exact either way.
//
// keyframe_culling_kernel: ONE workgroup of 1024 threads walks the local keyframes in the caller's order — the loop is sequential in
// the reference, a culled keyframe changes what the later ones see — with its threads over the slots of the current keyframe.  The
// state between keyframes is two byte arrays in global memory, removed[keyframe] and bad[point] (covis_math.hpp); a barrier with a
// device fence separates the keyframes.
//
// mappoint_culling_kernel: one thread per point.
//
// Host side: one staged upload and one download per call on the staging helpers of solver_host.hpp; nothing stays resident.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <stdexcept>

#include "common.hpp"
#include "solver_host.hpp"

#pragma clang fp contract(off)

#include "covis_math.hpp"

namespace sivo {

constexpr int CC_THREADS = 256;
constexpr int KC_THREADS = 1024;
constexpr int MC_THREADS = 256;

struct CcArgs {
    SivoObsTable t;                // device pointers
    const int64_t *set_off;
    const int32_t *set_point, *set_self;
    int32_t *counts;               // n_sets x n_kf; zeroed before the launch when n_kf > SIVO_COVIS_LDS_KF
};

__global__ __launch_bounds__(CC_THREADS) void covis_count_kernel(CcArgs a) {
    __shared__ int32_t hist[SIVO_COVIS_LDS_KF];
    const int s = blockIdx.x, tid = threadIdx.x, n_kf = a.t.n_kf;
    const int64_t s0 = a.set_off[s], s1 = a.set_off[s + 1];
    const int32_t self = a.set_self[s];
    int32_t *row = a.counts + (int64_t)s * n_kf;
    if (n_kf <= SIVO_COVIS_LDS_KF) {
        for (int k = tid; k < n_kf; k += CC_THREADS) hist[k] = 0;
        __syncthreads();
        for (int64_t i = s0 + tid; i < s1; i += CC_THREADS)
            cv_count_slot(a.t, a.set_point[i], self, [&](int32_t k) { atomicAdd(&hist[k], 1); });
        __syncthreads();
        for (int k = tid; k < n_kf; k += CC_THREADS) row[k] = hist[k];
    } else {
        for (int64_t i = s0 + tid; i < s1; i += CC_THREADS)
            cv_count_slot(a.t, a.set_point[i], self, [&](int32_t k) { atomicAdd(&row[k], 1); });
    }
}

struct KcArgs {
    SivoObsTable t;                // device pointers
    int n_local, monocular;
    const int32_t *local_kf;
    const uint8_t *is_id0, *erasable;
    const float *th_depth;
    const int64_t *slot_off;
    const int32_t *slot_point;
    const uint8_t *slot_level;
    const float *slot_depth;
    int32_t *n_mps, *n_red;
    uint8_t *decision;
    uint8_t *bad;                  // n_points: point_bad on entry of the loop, bad_after at its end
    uint8_t *removed;              // n_kf, zeroed before the launch
    uint8_t *slot_goes_bad;        // per slot, scratch: EraseObservation of the slot's keyframe would leave the point with nObs <= 2
};

__global__ __launch_bounds__(KC_THREADS) void keyframe_culling_kernel(KcArgs a) {
    __shared__ int32_t part[KC_THREADS / 64][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int p = tid; p < a.t.n_points; p += KC_THREADS) a.bad[p] = a.t.point_bad[p];
    __threadfence();
    __syncthreads();
    for (int j = 0; j < a.n_local; ++j) {
        if (a.is_id0[j]) {                                              // (LocalMapping.cc:735; the same for every thread)
            if (tid == 0) a.decision[j] = SIVO_KFCULL_ID0;
            continue;
        }
        const int32_t kf = a.local_kf[j];
        const int64_t s0 = a.slot_off[j], s1 = a.slot_off[j + 1];
        const float th = a.th_depth[j];
        int32_t mps = 0, red = 0;
        for (int64_t i = s0 + tid; i < s1; i += KC_THREADS) {
            const CvSlot r = cv_kf_slot(a.t, a.bad, a.removed, kf, a.slot_point[i], a.slot_level[i], a.slot_depth[i], th, a.monocular);
            mps += r.counted; red += r.redundant;
            a.slot_goes_bad[i] = (uint8_t)r.goes_bad;                   // read back below by the thread that wrote it
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { mps += __shfl_xor(mps, m, 64); red += __shfl_xor(red, m, 64); }
        if (lane == 0) { part[wave][0] = mps; part[wave][1] = red; }
        __syncthreads();
        mps = 0; red = 0;
#pragma unroll
        for (int w = 0; w < KC_THREADS / 64; ++w) { mps += part[w][0]; red += part[w][1]; }
        const uint8_t d = cv_kf_decision(red, mps, a.erasable[j]);      // (:789) the same in every thread
        if (tid == 0) { a.n_mps[j] = mps; a.n_red[j] = red; a.decision[j] = d; }
        if (d == SIVO_KFCULL_CULLED) {
            // KeyFrame::SetBadFlag (KeyFrame.cc:493-495): EraseObservation on every slot's point, by what the walk above found of it
            // (no state has changed since).  Nothing reads bad[] here; a point that sits in two slots is marked twice.
            for (int64_t i = s0 + tid; i < s1; i += KC_THREADS)
                if (a.slot_goes_bad[i]) a.bad[a.slot_point[i]] = 1;
            if (tid == 0) a.removed[kf] = 1;                            // (every walk of this keyframe ended before the barrier above)
        }
        __threadfence();
        __syncthreads();
    }
}

struct McArgs {
    int n, monocular;
    int64_t current_kf_id;
    const int32_t *found, *visible, *n_obs;
    const int64_t *first_kf_id;
    const uint8_t *bad;
    uint8_t *status;
};

__global__ __launch_bounds__(MC_THREADS) void mappoint_culling_kernel(McArgs a) {
    const int i = blockIdx.x * MC_THREADS + (int)threadIdx.x;
    if (i >= a.n) return;
    a.status[i] = cv_mappoint_status(a.found[i], a.visible[i], a.first_kf_id[i], a.n_obs[i], a.bad[i], a.current_kf_id, a.monocular);
}

static void cv_throw(const char *what, const char *e) {
    if (e) throw std::invalid_argument(std::string(what) + ": " + e);
}

// the table's arrays into the call's one upload
static void cv_stage_table(Layout &L, const SivoObsTable &t, SivoObsTable &d) {
    const size_t P = (size_t)t.n_points, no = P ? (size_t)t.obs_off[P] : 0;
    d.n_kf = t.n_kf; d.n_points = t.n_points;
    L.copy(d.obs_off, t.obs_off, P ? 8 * (P + 1) : 0); L.copy(d.obs_kf, t.obs_kf, 4 * no); L.copy(d.obs_level, t.obs_level, no);
    L.copy(d.obs_stereo, t.obs_stereo, no); L.copy(d.point_bad, t.point_bad, P);
}

static SolverCtx &cv_ctx() {
    static thread_local SolverCtx c(false, 4 << 20, 0, 4 << 20);
    c.bind();
    return c;
}

}  // namespace sivo

using namespace sivo;

extern "C" int sivo_covis_count(const SivoObsTable *t, int n_sets, const int64_t *set_off, const int32_t *set_point,
                                const int32_t *set_self, int32_t *counts) {
    return guarded([&] {
        cv_throw("sivo_covis_count", cv_check_count(t, n_sets, set_off, set_point, set_self, counts));
        if (n_sets == 0 || t->n_kf == 0) return SIVO_OK;
        const size_t S = (size_t)n_sets, ns = (size_t)set_off[S], nc = S * (size_t)t->n_kf;
        if (ns == 0) {                                                  // no slot anywhere: nothing to launch
            std::memset(counts, 0, 4 * nc);
            return SIVO_OK;
        }
        require_device();
        SolverCtx &c = cv_ctx();
        CcArgs a;
        Layout L;
        cv_stage_table(L, *t, a.t);
        L.copy(a.set_off, set_off, 8 * (S + 1)); L.copy(a.set_point, set_point, 4 * ns); L.copy(a.set_self, set_self, 4 * S);
        if (t->n_kf > SIVO_COVIS_LDS_KF) L.zero(a.counts, 4 * nc);
        else L.take(a.counts, 4 * nc);
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        L.send(c.stream);
        hipLaunchKernelGGL(covis_count_kernel, dim3((unsigned)n_sets), dim3(CC_THREADS), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipMemcpyAsync(L.host(a.counts), a.counts, 4 * nc, hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        std::memcpy(counts, L.host(a.counts), 4 * nc);
        return SIVO_OK;
    });
}

extern "C" int sivo_keyframe_culling(const SivoObsTable *t, int n_local, const int32_t *local_kf, const uint8_t *is_id0,
                                     const uint8_t *erasable, const float *th_depth, const int64_t *slot_off,
                                     const int32_t *slot_point, const uint8_t *slot_level, const float *slot_depth, int monocular,
                                     int32_t *n_mps, int32_t *n_redundant, uint8_t *decision, uint8_t *bad_after) {
    return guarded([&] {
        cv_throw("sivo_keyframe_culling", cv_check_kfcull(t, n_local, local_kf, is_id0, erasable, th_depth, slot_off, slot_point, slot_level,
                                                          slot_depth, n_mps, n_redundant, decision, bad_after));
        const size_t P = (size_t)t->n_points, K = (size_t)n_local;
        if (n_local == 0) {                                             // no keyframe: no point changes
            if (P) std::memcpy(bad_after, t->point_bad, P);
            return SIVO_OK;
        }
        require_device();
        SolverCtx &c = cv_ctx();
        const size_t ns = (size_t)slot_off[K];
        KcArgs a;
        Layout L;
        cv_stage_table(L, *t, a.t);
        L.copy(a.local_kf, local_kf, 4 * K); L.copy(a.is_id0, is_id0, K); L.copy(a.erasable, erasable, K); L.copy(a.th_depth, th_depth, 4 * K);
        L.copy(a.slot_off, slot_off, 8 * (K + 1)); L.copy(a.slot_point, slot_point, 4 * ns); L.copy(a.slot_level, slot_level, ns);
        L.copy(a.slot_depth, slot_depth, 4 * ns);
        L.zero(a.removed, (size_t)t->n_kf);
        L.take(a.n_mps, 4 * K); L.take(a.n_red, 4 * K); L.take(a.decision, K); L.take(a.bad, P);
        L.take(a.slot_goes_bad, ns);                                    // scratch behind the results: not copied back
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        a.n_local = n_local; a.monocular = monocular != 0;
        L.send(c.stream);
        hipLaunchKernelGGL(keyframe_culling_kernel, dim3(1), dim3(KC_THREADS), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipMemcpyAsync(L.host(a.n_mps), a.n_mps, (size_t)((const char *)a.bad - (const char *)a.n_mps) + P, hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        const int32_t *hm = L.host(a.n_mps), *hr = L.host(a.n_red);
        const uint8_t *hd = L.host(a.decision);
        for (size_t j = 0; j < K; ++j) {
            decision[j] = hd[j];
            if (hd[j] == SIVO_KFCULL_ID0) continue;                     // its counts are not written
            n_mps[j] = hm[j]; n_redundant[j] = hr[j];
        }
        if (P) std::memcpy(bad_after, L.host(a.bad), P);
        return SIVO_OK;
    });
}

extern "C" int sivo_mappoint_culling(int n, const int32_t *found, const int32_t *visible, const int64_t *first_kf_id,
                                     const int32_t *n_obs, const uint8_t *bad, int64_t current_kf_id, int monocular, uint8_t *status) {
    return guarded([&] {
        cv_throw("sivo_mappoint_culling", cv_check_mpcull(n, found, visible, first_kf_id, n_obs, bad, status));
        if (n == 0) return SIVO_OK;
        require_device();
        SolverCtx &c = cv_ctx();
        const size_t N = (size_t)n;
        McArgs a;
        Layout L;
        L.copy(a.found, found, 4 * N); L.copy(a.visible, visible, 4 * N); L.copy(a.n_obs, n_obs, 4 * N);
        L.copy(a.first_kf_id, first_kf_id, 8 * N); L.copy(a.bad, bad, N);
        L.take(a.status, N);
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        a.n = n; a.monocular = monocular != 0; a.current_kf_id = current_kf_id;
        L.send(c.stream);
        hipLaunchKernelGGL(mappoint_culling_kernel, dim3((unsigned)cdiv(n, MC_THREADS)), dim3(MC_THREADS), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipMemcpyAsync(L.host(a.status), a.status, L.results(), hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        std::memcpy(status, L.host(a.status), N);
        return SIVO_OK;
    });
}
