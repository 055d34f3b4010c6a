// localmap_track.hip — Tracking::TrackLocalMap's two device halves in one call (reference src/orbslam/Tracking.cc:1033-1124): the resident
// map keeps the map points' attributes beside its integer graph, so the mvpLocalMapPoints that sivo_localmap_update leaves on the device
// feed Tracking::SearchLocalPoints without a walk over MapPoint objects on the host, without a second upload of local_point and without
// a per-point host array.  The per-item bodies and the argument checks are localmap_track_math.hpp.
//
// The attribute store (sivo_localmap_set_points / _get_points): structure-of-arrays over the handle's point indices in an allocation of
// the handle's own (localmap_handle.hpp), one upload of the caller's rows and
// localmap_attr_scatter_kernel  one thread per row of the upload: the row into the store (the indices are strictly increasing: no two
//                               threads write one row).
// localmap_attr_gather_kernel   one thread per row asked for: the row out of the store.
//
// sivo_localmap_search_local_points: the update runs as sivo_localmap_update runs it (lm_run_update of localmap.hip: the same upload,
// launches, download and synchronisation), with seen_point added to the upload and, behind the point passes,
// localmap_skip_mark_kernel     one thread per frame slot and per seen_point: first[p] = LM_FIRST_PREMARKED where the second loop of
//                               SearchLocalPoints would find mnLastFrameSeen == the frame's id (plain stores of one value).
// Then the search engine of search.hip runs on the frame with a producer (DeviceQueries, search_engine.hpp) whose kernel
// localmap_track_queries_kernel one thread per local point i: reads local_point[i] and its stored row, runs fr_point / fr_query /
//                               fr_no_query of frustum_math.hpp and writes the query record, the 32-byte descriptor, status and the track
//                               fields; the same threads, one per keypoint, write the engine's blocked flags from frame_point,
//                               slot_cleared and n_obs.  LDS-free; the reads of a row are a gather by point index (12 + 12 + 4 + 4 + 4 +
//                               32 bytes from six arrays), the writes are coalesced.
// The queries, their descriptors and the flags live in the engine's device-only scratch: the engine's upload holds its own initial
// values only, its download the matches, status and the track fields.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "localmap_handle.hpp"
#include "search_engine.hpp"

namespace sivo {
namespace {

struct LtRowCall {
    LtAttrs at;
    LtRows r;
};

__global__ __launch_bounds__(LP_THREADS) void localmap_attr_scatter_kernel(LtRowCall a) {
    const int j = blockIdx.x * LP_THREADS + (int)threadIdx.x;
    if (j < a.r.n) lt_scatter_row(a.at, a.r, j);
}

__global__ __launch_bounds__(LP_THREADS) void localmap_attr_gather_kernel(LtRowCall a) {
    const int j = blockIdx.x * LP_THREADS + (int)threadIdx.x;
    if (j < a.r.n) lt_gather_row(a.at, a.r, j);
}

struct LtMarkCall {
    uint32_t *first;
    int32_t n_slots, n_seen;
    const int32_t *frame_point, *seen_point;
    const uint8_t *slot_cleared;
};

__global__ __launch_bounds__(LP_THREADS) void localmap_skip_mark_kernel(LtMarkCall a) {
    const int item = blockIdx.x * LP_THREADS + (int)threadIdx.x;
    if (item < a.n_slots + a.n_seen) lt_mark_skip(a.first, a.n_slots, a.frame_point, a.slot_cleared, a.n_seen, a.seen_point, item);
}

__global__ __launch_bounds__(LP_THREADS) void localmap_track_queries_kernel(LtProduce a) {
    const int t = blockIdx.x * LP_THREADS + (int)threadIdx.x;
    if (t < a.n) lt_produce_point(a, t);
    if (t < a.n_keys) a.blocked[t] = lt_blocked(a.frame_point, a.slot_cleared, a.at.n_obs, t);
}

// seen_point into the update's upload, the skip mark behind its point passes
struct SkipMark : LmUpdateHook {
    int n_seen;
    const int32_t *seen_point, *d_seen = nullptr;
    SkipMark(int n, const int32_t *s) : n_seen(n), seen_point(s) {}
    void regions(Layout &L) override { L.copy(d_seen, seen_point, 4 * (size_t)n_seen); }
    void launch(const LmCall &a, hipStream_t stream) override {
        const LtMarkCall k{a.first, a.n_slots, n_seen, a.frame_point, d_seen, a.slot_cleared};
        const int items = a.n_slots + n_seen;
        if (items == 0) return;
        hipLaunchKernelGGL(localmap_skip_mark_kernel, dim3((unsigned)cdiv(items, LP_THREADS)), dim3(LP_THREADS), 0, stream, k);
        SIVO_HIP(hipGetLastError());
    }
};

// the engine's producer: the queries of local_point[0 .. n) from the store
struct TrackQueries : DeviceQueries {
    LtProduce a;
    uint8_t *status;
    float *px, *py, *pxr, *vc;                             // the caller's; each may be null
    int32_t *level;
    int n_to_match = 0;
    bool device_inputs() const override { return true; }
    void regions(Layout &L) override {
        const size_t N = (size_t)a.n;
        L.take(a.status, N); L.take(a.px, 4 * N); L.take(a.py, 4 * N); L.take(a.pxr, 4 * N); L.take(a.vc, 4 * N); L.take(a.level, 4 * N);
    }
    void launch(const sivo_mframe &F, const EngineRegions &r) override {
        a.scale = F.view().scale;                                  // (after scratch(): the frame may have moved to a bigger slab)
        a.q = r.q; a.qdesc = (uint32_t *)r.qdesc; a.blocked = r.blocked;
        hipLaunchKernelGGL(localmap_track_queries_kernel, dim3((unsigned)cdiv(std::max(a.n, a.n_keys), LP_THREADS)), dim3(LP_THREADS), 0,
                           F.stream, a);
        SIVO_HIP(hipGetLastError());
    }
    void collect(const Layout &L) override {
        const uint8_t *hs = L.host(a.status);
        const float *hx = L.host(a.px), *hy = L.host(a.py), *hr = L.host(a.pxr), *hc = L.host(a.vc);
        const int32_t *hl = L.host(a.level);
        for (int32_t i = 0; i < a.n; ++i) {
            status[i] = hs[i];
            if (hs[i] != SIVO_FRUSTUM_IN_VIEW) continue;               // nothing else of the point is written
            ++n_to_match;
            if (px) px[i] = hx[i];
            if (py) py[i] = hy[i];
            if (pxr) pxr[i] = hr[i];
            if (vc) vc[i] = hc[i];
            if (level) level[i] = hl[i];
        }
    }
};

void lt_throw(const char *what, const std::string &e) {
    if (!e.empty()) throw std::invalid_argument(std::string(what) + ": " + e);
}

}  // namespace
}  // namespace sivo

using namespace sivo;

extern "C" int sivo_localmap_set_points(sivo_localmap_t m, int n_rows, const int32_t *point_idx, const float *pos, const float *normal,
                                        const float *min_dist, const float *max_dist, const uint8_t *desc, const int32_t *n_obs) {
    return guarded([&] {
        if (!m) throw std::invalid_argument("sivo_localmap_set_points: null handle");
        std::lock_guard<std::mutex> lock(m->mu);
        lt_throw("sivo_localmap_set_points", lt_check_set_points(m->d.n_points, n_rows, point_idx, pos, normal, min_dist, max_dist, desc, n_obs));
        if (n_rows == 0) return SIVO_OK;
        require_device();
        DeviceGuard dg(m->device);
        SolverCtx &c = lm_ctx();
        const size_t R = (size_t)n_rows;
        LtRowCall a;
        a.at = m->attr; a.r.n = n_rows;
        Layout L;
        L.copy(a.r.idx, point_idx, 4 * R); L.copy(a.r.pos, pos, 12 * R); L.copy(a.r.normal, normal, 12 * R);
        L.copy(a.r.min_dist, min_dist, 4 * R); L.copy(a.r.max_dist, max_dist, 4 * R); L.copy(a.r.desc, desc, 32 * R); L.copy(a.r.n_obs, n_obs, 4 * R);
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        L.send(c.stream);
        hipLaunchKernelGGL(localmap_attr_scatter_kernel, dim3((unsigned)cdiv(n_rows, LP_THREADS)), dim3(LP_THREADS), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipStreamSynchronize(c.stream));
        for (int i = 0; i < n_rows; ++i) {
            const int32_t p = point_idx[i];
            if (!m->attr_is_set(p)) { m->attr_set[(size_t)p >> 6] |= (uint64_t)1 << (p & 63); ++m->n_attr_set; }
        }
        return SIVO_OK;
    });
}

extern "C" int sivo_localmap_get_points(sivo_localmap_t m, int n_rows, const int32_t *point_idx, float *pos, float *normal, float *min_dist,
                                        float *max_dist, uint8_t *desc, int32_t *n_obs, uint8_t *is_set) {
    return guarded([&] {
        if (!m) throw std::invalid_argument("sivo_localmap_get_points: null handle");
        std::lock_guard<std::mutex> lock(m->mu);
        lt_throw("sivo_localmap_get_points", lt_check_get_points(m->d.n_points, n_rows, point_idx, pos, normal, min_dist, max_dist, desc, n_obs, is_set));
        if (n_rows == 0) return SIVO_OK;
        require_device();
        DeviceGuard dg(m->device);
        SolverCtx &c = lm_ctx();
        const size_t R = (size_t)n_rows;
        LtRowCall a;
        a.at = m->attr; a.r.n = n_rows;
        Layout L;
        L.copy(a.r.idx, point_idx, 4 * R);
        L.take(a.r.pos, 12 * R); L.take(a.r.normal, 12 * R); L.take(a.r.min_dist, 4 * R); L.take(a.r.max_dist, 4 * R); L.take(a.r.desc, 32 * R);
        L.take(a.r.n_obs, 4 * R);
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        L.send(c.stream);
        hipLaunchKernelGGL(localmap_attr_gather_kernel, dim3((unsigned)cdiv(n_rows, LP_THREADS)), dim3(LP_THREADS), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipMemcpyAsync(L.host(a.r.pos), a.r.pos, L.results(), hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        std::memcpy(pos, L.host(a.r.pos), 12 * R); std::memcpy(normal, L.host(a.r.normal), 12 * R);
        std::memcpy(min_dist, L.host(a.r.min_dist), 4 * R); std::memcpy(max_dist, L.host(a.r.max_dist), 4 * R);
        std::memcpy(desc, L.host(a.r.desc), 32 * R); std::memcpy(n_obs, L.host(a.r.n_obs), 4 * R);
        for (int i = 0; i < n_rows; ++i) {                              // a row nobody set reads as zeros, whatever the allocation holds
            is_set[i] = m->attr_is_set(point_idx[i]) ? 1 : 0;
            if (is_set[i]) continue;
            std::memset(pos + 3 * (size_t)i, 0, 12); std::memset(normal + 3 * (size_t)i, 0, 12); std::memset(desc + 32 * (size_t)i, 0, 32);
            min_dist[i] = 0.0f; max_dist[i] = 0.0f; n_obs[i] = 0;
        }
        return SIVO_OK;
    });
}

extern "C" int sivo_localmap_search_local_points(sivo_localmap_t m, sivo_mframe_t F, const SivoFrustum *frustum, int n_slots,
                                                 const int32_t *frame_point, int n_kf_premarked, const int32_t *kf_premarked,
                                                 int n_point_premarked, const int32_t *point_premarked, int n_prev,
                                                 const int32_t *prev_local_kf, int n_seen, const int32_t *seen_point, float th, float nn_ratio,
                                                 int32_t *voted, uint8_t *slot_cleared, int kf_capacity, int32_t *local_kf, int32_t *n_local_kf,
                                                 int32_t *ref_kf, int point_capacity, int32_t *local_point, int32_t *n_local_points,
                                                 int32_t *counts, uint8_t *status, float *proj_x, float *proj_y, float *proj_xr, float *view_cos,
                                                 int32_t *level, int32_t *match, int *n_to_match, int *n_matches) {
    return guarded([&] {
        const char *who = "sivo_localmap_search_local_points";
        if (!m) throw std::invalid_argument(std::string(who) + ": null handle");
        if (!F) throw std::invalid_argument(std::string(who) + ": null frame");
        std::lock_guard<std::mutex> lock(m->mu);
        int64_t g_prev = 0;
        lm_throw(who, lm_check_update(m->d.n_kf, m->d.n_points, m->slot_off.data(), n_slots, frame_point, n_kf_premarked, kf_premarked,
                                      n_point_premarked, point_premarked, n_prev, prev_local_kf, voted, slot_cleared, kf_capacity, local_kf,
                                      n_local_kf, ref_kf, point_capacity, local_point, n_local_points, &g_prev));
        lt_throw(who, lt_check_search(m->device, F->device, F->n, F->nlevels, frustum, n_slots, m->d.n_points, m->attr_set.data(), m->n_attr_set,
                                      n_seen, seen_point, point_capacity, status, match));
        TrackQueries tq;
        if (!fr_camera(*frustum, tq.a.cam)) throw std::invalid_argument(std::string(who) + ": log_scale_factor must be positive");
        const LmUpdateArgs u{n_slots, frame_point, n_kf_premarked, kf_premarked, n_point_premarked, point_premarked, n_prev, prev_local_kf, voted,
                             slot_cleared, kf_capacity, local_kf, n_local_kf, ref_kf, point_capacity, local_point, n_local_points, counts};
        SkipMark mark(n_seen, seen_point);
        LmCall call;
        const int rc = lm_run_update(m, u, g_prev, who, &mark, &call);
        if (rc != SIVO_OK) return rc;                                   // SIVO_ERR_CAPACITY: nothing of the search is written
        const int32_t np = *n_local_points;
        tq.a.th = th; tq.a.n = np; tq.a.local_point = call.local_point; tq.a.first = m->first; tq.a.at = m->attr; tq.a.scale = nullptr;
        tq.a.n_keys = n_slots; tq.a.frame_point = call.frame_point; tq.a.slot_cleared = call.slot_cleared;
        tq.status = status; tq.px = proj_x; tq.py = proj_y; tq.pxr = proj_xr; tq.vc = view_cos; tq.level = level;
        const SivoSearchRule rule = make_rule(SIVO_TH_HIGH, 1, 1, nn_ratio, false, true);
        run_search(*F, nullptr, nullptr, np, nullptr, nullptr, nullptr, 0, rule, nullptr, nullptr, match, nullptr, nullptr, n_matches, nullptr, &tq);
        if (n_to_match) *n_to_match = tq.n_to_match;
        return SIVO_OK;
    });
}
