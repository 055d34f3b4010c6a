// frustum_host_capi.hpp — sivo_frustum_cull and sivo_search_local_points of include/sivo_hip.h over the HOST build of the kernels' arithmetic
// (sivo_amd/csrc/frustum_math.hpp), with the results stored as frustum.hip and search.hip store them (the entries of a point that is not
// in view left as the caller had them), and the few other entry points SIVO::SearchLocalPoints (sivo_amd/api/orbslam/TrackingAdapter.h)
// reaches: a frame view that only keeps the arrays, and the matching of ORBmatcher::SearchByProjection(Frame &, const vector<MapPoint *> &,
// th) (reference src/orbslam/ORBmatcher.cc:44-127) as the sequential loop it is, over the queries fr_query makes.  tests/frustum_prog.cpp
// includes it, so the program needs neither the library nor a device and can run under the sanitizers.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "frustum_math.hpp"

struct sivo_mframe {
    std::vector<SivoKeyPoint> keys;
    std::vector<float> u_right, scale;
    std::vector<uint8_t> desc;
    float min_x, max_x, min_y, max_y;
    int nlevels;
};

namespace frustum_host {
inline std::string &error() { static std::string e; return e; }
inline int fail(const char *what) { error() = what; return SIVO_ERR_INVALID_ARGUMENT; }

// Frame::GetFeaturesInArea (Frame.cc:326-390) without the grid: the cells are visited column by column, the keys of a cell in index order
inline void features_in_area(const sivo_mframe &F, float x, float y, float r, int minLevel, int maxLevel, std::vector<int> &out) {
    const int COLS = 64, ROWS = 48;
    const float inv_w = (float)COLS / (F.max_x - F.min_x), inv_h = (float)ROWS / (F.max_y - F.min_y);
    out.clear();
    const int x0 = std::max(0, (int)std::floor((x - F.min_x - r) * inv_w));
    if (x0 >= COLS) return;
    const int x1 = std::min(COLS - 1, (int)std::ceil((x - F.min_x + r) * inv_w));
    if (x1 < 0) return;
    const int y0 = std::max(0, (int)std::floor((y - F.min_y - r) * inv_h));
    if (y0 >= ROWS) return;
    const int y1 = std::min(ROWS - 1, (int)std::ceil((y - F.min_y + r) * inv_h));
    if (y1 < 0) return;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = x0; ix <= x1; ++ix)
        for (int iy = y0; iy <= y1; ++iy)
            for (size_t k = 0; k < F.keys.size(); ++k) {
                const SivoKeyPoint &kp = F.keys[k];
                const int px = (int)std::round((kp.x - F.min_x) * inv_w), py = (int)std::round((kp.y - F.min_y) * inv_h);
                if (px != ix || py != iy) continue;
                if (bCheckLevels) {
                    if (kp.octave < minLevel) continue;
                    if (maxLevel >= 0 && kp.octave > maxLevel) continue;
                }
                if (std::fabs(kp.x - x) < r && std::fabs(kp.y - y) < r) out.push_back((int)k);
            }
}

inline int distance(const uint8_t *a, const uint8_t *b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}
}  // namespace frustum_host

extern "C" {

const char *sivo_last_error(void) { return frustum_host::error().c_str(); }

int sivo_mframe_create(const SivoKeyPoint *keys, int n, const float *u_right, const uint8_t *descriptors, float min_x, float max_x, float min_y,
                       float max_y, const float *scale_factors, const float *, const float *, int nlevels, int, sivo_mframe_t *out) {
    if (!out || n < 0 || nlevels < 1) return frustum_host::fail("sivo_mframe_create");
    sivo_mframe *F = new sivo_mframe;
    F->keys.assign(keys, keys + n);
    F->u_right.assign((size_t)n, -1.0f);
    if (u_right) F->u_right.assign(u_right, u_right + n);
    F->desc.assign(descriptors, descriptors + 32 * (size_t)n);
    F->scale.assign(scale_factors, scale_factors + nlevels);
    F->min_x = min_x; F->max_x = max_x; F->min_y = min_y; F->max_y = max_y; F->nlevels = nlevels;
    *out = F;
    return SIVO_OK;
}

int sivo_mframe_destroy(sivo_mframe_t h) {
    delete h;
    return SIVO_OK;
}

int sivo_frustum_cull(const SivoFrustum *frustum, int n, const float *pos, const float *normal, const float *min_dist, const float *max_dist,
                      const uint8_t *skip, uint8_t *status, float *proj_x, float *proj_y, float *proj_xr, float *view_cos, int32_t *level,
                      int *n_in_view) {
    sivo::FrCamera cam;
    if (!frustum || n < 0 || !sivo::fr_camera(*frustum, cam)) return frustum_host::fail("sivo_frustum_cull: frustum");
    if (n_in_view) *n_in_view = 0;
    if (n > 0 && (!pos || !normal || !min_dist || !max_dist || !status || !proj_x || !proj_y || !proj_xr || !view_cos || !level))
        return frustum_host::fail("sivo_frustum_cull: null argument");
    for (int i = 0; i < n; ++i) {
        sivo::FrResult o;
        status[i] = skip && skip[i] ? (uint8_t)SIVO_FRUSTUM_SKIPPED : sivo::fr_point(cam, pos + 3 * i, normal + 3 * i, min_dist[i], max_dist[i], o);
        if (status[i] != SIVO_FRUSTUM_IN_VIEW) continue;
        proj_x[i] = o.u; proj_y[i] = o.v; proj_xr[i] = o.ur; view_cos[i] = o.view_cos; level[i] = o.level;
        if (n_in_view) ++*n_in_view;
    }
    return SIVO_OK;
}

int sivo_search_local_points(sivo_mframe_t F, const SivoFrustum *frustum, int n, const float *pos, const float *normal, const float *min_dist,
                             const float *max_dist, const uint8_t *skip, const uint8_t *mp_desc, const int32_t *mp_obs, float th, float nn_ratio,
                             int32_t *occ_obs, int32_t *match, uint8_t *status, float *proj_x, float *proj_y, float *proj_xr, float *view_cos,
                             int32_t *level, int *n_to_match, int *n_matches) {
    sivo::FrCamera cam;
    if (!F || !frustum || n < 0 || !occ_obs || !match || !sivo::fr_camera(*frustum, cam) || frustum->nlevels > F->nlevels)
        return frustum_host::fail("sivo_search_local_points: frustum");
    if (n > 0 && (!pos || !normal || !min_dist || !max_dist || !mp_desc || !mp_obs || !status)) return frustum_host::fail("sivo_search_local_points: null argument");
    const int nk = (int)F->keys.size();
    for (int k = 0; k < nk; ++k) match[k] = -1;
    int to_match = 0, nmatches = 0;
    std::vector<int> cand;
    for (int i = 0; i < n; ++i) {
        sivo::FrResult o;
        status[i] = skip && skip[i] ? (uint8_t)SIVO_FRUSTUM_SKIPPED : sivo::fr_point(cam, pos + 3 * i, normal + 3 * i, min_dist[i], max_dist[i], o);
        if (status[i] != SIVO_FRUSTUM_IN_VIEW) continue;
        ++to_match;
        if (proj_x) proj_x[i] = o.u;
        if (proj_y) proj_y[i] = o.v;
        if (proj_xr) proj_xr[i] = o.ur;
        if (view_cos) view_cos[i] = o.view_cos;
        if (level) level[i] = o.level;
        SivoSearchQuery q;
        sivo::fr_query(o, th, F->scale.data(), mp_obs[i], q);
        frustum_host::features_in_area(*F, q.u, q.v, q.radius, q.lvl_lo, q.lvl_hi, cand);
        int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;       // ORBmatcher.cc:79-113
        for (int idx : cand) {
            if (occ_obs[idx] > 0) continue;
            if (F->u_right[(size_t)idx] > 0) {
                const float er = std::fabs(q.ur - F->u_right[(size_t)idx]);
                if (er > q.gate) continue;
            }
            const int dist = frustum_host::distance(mp_desc + 32 * (size_t)i, F->desc.data() + 32 * (size_t)idx);
            if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = F->keys[(size_t)idx].octave; bestIdx = idx; }
            else if (dist < bestDist2) { bestLevel2 = F->keys[(size_t)idx].octave; bestDist2 = dist; }
        }
        if (bestDist <= 100) {                                                                     // TH_HIGH (:117-123)
            if (bestLevel == bestLevel2 && (float)bestDist > nn_ratio * (float)bestDist2) continue;
            match[bestIdx] = i; occ_obs[bestIdx] = mp_obs[i];
            ++nmatches;
        }
    }
    if (n_to_match) *n_to_match = to_match;
    if (n_matches) *n_matches = nmatches;
    return SIVO_OK;
}

}  // extern "C"
