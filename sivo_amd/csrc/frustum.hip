// frustum.hip — Frame::isInFrustum (reference src/orbslam/Frame.cc:267-324) for the whole local map at once: the second loop of
// Tracking::SearchLocalPoints (Tracking.cc:1054-1070), which the tracking thread walks on every frame between its two pose optimisations.
// A few thousand points, each independent of every other: one thread per point, workgroups of 256; the camera (pose, intrinsics, image
// bounds, the level thresholds) is a kernel argument and so lives in scalar registers.  Latency bound, like triangulate.hip.
//
// Arithmetic: frustum_math.hpp, which g++ also compiles for the host (tests/frustum_prog.cpp); no logarithm is taken on the device.
// The fused form that writes the search engine's queries from the same function is fr_queries_kernel in search.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <stdexcept>

#include "common.hpp"
#include "solver_host.hpp"

#pragma clang fp contract(off)

#include "frustum_math.hpp"

namespace sivo {

constexpr int FR_THREADS = 256;

struct FrArgs {
    FrCamera cam;
    int n;
    const float *pos, *normal, *min_dist, *max_dist;
    const uint8_t *skip;           // may be null
    uint8_t *status;
    float *px, *py, *pxr, *vc;     // written for the points in view only
    int32_t *level;
    int32_t *count;                // may be null; zeroed before the launch
};

__global__ __launch_bounds__(FR_THREADS) void frustum_cull_kernel(FrArgs a) {
    const int i = blockIdx.x * FR_THREADS + (int)threadIdx.x;
    bool in_view = false;
    if (i < a.n) {
        uint8_t st = SIVO_FRUSTUM_SKIPPED;
        FrResult o;
        if (!(a.skip && a.skip[i])) {
            const float X[3] = {a.pos[3 * (int64_t)i], a.pos[3 * (int64_t)i + 1], a.pos[3 * (int64_t)i + 2]};
            const float N[3] = {a.normal[3 * (int64_t)i], a.normal[3 * (int64_t)i + 1], a.normal[3 * (int64_t)i + 2]};
            st = fr_point(a.cam, X, N, a.min_dist[i], a.max_dist[i], o);
        }
        a.status[i] = st;
        if (st == SIVO_FRUSTUM_IN_VIEW) {
            in_view = true;
            a.px[i] = o.u; a.py[i] = o.v; a.pxr[i] = o.ur; a.vc[i] = o.view_cos; a.level[i] = o.level;
        }
    }
    if (a.count) {                 // (uniform: every lane of the wave reaches the ballot)
        const unsigned long long m = __ballot(in_view);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.count, __popcll(m));
    }
}

static void fr_camera_or_throw(const SivoFrustum *f, FrCamera &cam) {
    if (!f) throw std::invalid_argument("null argument");
    if (f->nlevels < 1 || f->nlevels > 16) throw std::invalid_argument("nlevels outside 1 .. 16");
    if (!fr_camera(*f, cam)) throw std::invalid_argument("log_scale_factor must be positive");
}

}  // namespace sivo

using namespace sivo;

extern "C" int sivo_frustum_cull_dev(const SivoFrustum *frustum, int n, const float *d_pos, const float *d_normal,
                                     const float *d_min_dist, const float *d_max_dist, const uint8_t *d_skip, uint8_t *d_status,
                                     float *d_proj_x, float *d_proj_y, float *d_proj_xr, float *d_view_cos, int32_t *d_level,
                                     int32_t *d_n_in_view, void *stream) {
    return guarded([&] {
        if (n < 0 || n > (1 << 24)) throw std::invalid_argument("point count out of range");
        FrArgs a;
        fr_camera_or_throw(frustum, a.cam);
        if (n > 0 && (!d_pos || !d_normal || !d_min_dist || !d_max_dist || !d_status || !d_proj_x || !d_proj_y || !d_proj_xr || !d_view_cos || !d_level))
            throw std::invalid_argument("null argument");
        hipStream_t st = (hipStream_t)stream;
        if (d_n_in_view) SIVO_HIP(hipMemsetAsync(d_n_in_view, 0, 4, st));
        if (n == 0) return SIVO_OK;
        a.n = n; a.pos = d_pos; a.normal = d_normal; a.min_dist = d_min_dist; a.max_dist = d_max_dist; a.skip = d_skip;
        a.status = d_status; a.px = d_proj_x; a.py = d_proj_y; a.pxr = d_proj_xr; a.vc = d_view_cos; a.level = d_level;
        a.count = d_n_in_view;
        hipLaunchKernelGGL(frustum_cull_kernel, dim3((unsigned)cdiv(n, FR_THREADS)), dim3(FR_THREADS), 0, st, a);
        SIVO_HIP(hipGetLastError());
        return SIVO_OK;
    });
}

extern "C" int sivo_frustum_cull(const SivoFrustum *frustum, int n, const float *pos, const float *normal, const float *min_dist,
                                 const float *max_dist, const uint8_t *skip, uint8_t *status, float *proj_x, float *proj_y,
                                 float *proj_xr, float *view_cos, int32_t *level, int *n_in_view) {
    return guarded([&] {
        if (n < 0 || n > (1 << 24)) throw std::invalid_argument("point count out of range");
        FrArgs a;
        fr_camera_or_throw(frustum, a.cam);
        if (n_in_view) *n_in_view = 0;
        if (n == 0) return SIVO_OK;
        if (!pos || !normal || !min_dist || !max_dist || !status || !proj_x || !proj_y || !proj_xr || !view_cos || !level)
            throw std::invalid_argument("null argument");
        require_device();
        // the tracking thread culls once per frame: pinned staging and device buffers kept per thread.  One copy up (the points), one
        // launch, one copy down (status and the track fields), one synchronisation.
        static thread_local SolverCtx c(true, 256 << 10, 0, 256 << 10);
        c.bind();
        const size_t N = (size_t)n;
        Layout L;
        L.copy(a.pos, pos, 12 * N); L.copy(a.normal, normal, 12 * N); L.copy(a.min_dist, min_dist, 4 * N); L.copy(a.max_dist, max_dist, 4 * N);
        if (skip) L.copy(a.skip, skip, N);
        else a.skip = nullptr;
        L.take(a.status, N); L.take(a.px, 4 * N); L.take(a.py, 4 * N); L.take(a.pxr, 4 * N); L.take(a.vc, 4 * N); L.take(a.level, 4 * N);
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        a.n = n; a.count = nullptr;
        L.send(c.stream);
        hipLaunchKernelGGL(frustum_cull_kernel, dim3((unsigned)cdiv(n, FR_THREADS)), dim3(FR_THREADS), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipMemcpyAsync(L.host(a.status), a.status, L.results(), hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        const uint8_t *hs = L.host(a.status);
        const float *hx = L.host(a.px), *hy = L.host(a.py), *hr = L.host(a.pxr), *hc = L.host(a.vc);
        const int32_t *hl = L.host(a.level);
        int count = 0;
        for (size_t i = 0; i < N; ++i) {
            status[i] = hs[i];
            if (hs[i] != SIVO_FRUSTUM_IN_VIEW) continue;               // nothing else of the point is written
            proj_x[i] = hx[i]; proj_y[i] = hy[i]; proj_xr[i] = hr[i]; view_cos[i] = hc[i]; level[i] = hl[i];
            ++count;
        }
        if (n_in_view) *n_in_view = count;
        return SIVO_OK;
    });
}
