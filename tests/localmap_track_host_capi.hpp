// localmap_track_host_capi.hpp — sivo_localmap_set_points, _get_points and _search_local_points of include/sivo_hip.h over the HOST build of
// the kernels' per-item bodies (sivo_amd/csrc/localmap_track_math.hpp), on top of localmap_host_capi.hpp / localmap_delta_host_capi.hpp
// (the handle, the update, apply) and frustum_host_capi.hpp (the frame view and the window walk), which it includes unchanged.  The
// attribute store lives beside the base handle; create, replace, apply and destroy are wrapped to keep its lifetime rules.  The call
// itself walks what localmap_track.hip launches: the update, the skip mark over first[], the producer per local point and per keypoint,
// and then ORBmatcher::SearchByProjection (reference src/orbslam/ORBmatcher.cc:79-123) as the sequential loop it is, over the queries the
// producer wrote.  No library, no device: the programs that include it run under the sanitizers.
#pragma once
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// the two base headers each define sivo_last_error: the frame view's is set aside, the handle's serves this header too
#define sivo_last_error frustum_host_last_error
#include "frustum_host_capi.hpp"
#undef sivo_last_error
// the entry points whose host versions must also keep the store: the base versions under another name
#define sivo_localmap_create localmap_base_create
#define sivo_localmap_replace localmap_base_replace
#define sivo_localmap_destroy localmap_base_destroy
#define sivo_localmap_apply localmap_base_apply
#include "localmap_delta_host_capi.hpp"
#undef sivo_localmap_create
#undef sivo_localmap_replace
#undef sivo_localmap_destroy
#undef sivo_localmap_apply

#include "localmap_track_math.hpp"

namespace localmap_track_host {
struct Store {
    std::vector<float> pos, normal, min_dist, max_dist;
    std::vector<uint32_t> desc;
    std::vector<int32_t> n_obs;
    std::vector<uint64_t> set;
    int64_t n_set = 0;
    void resize(size_t P) {                    // the rows it holds stay; new rows are unset
        pos.resize(3 * P); normal.resize(3 * P); min_dist.resize(P); max_dist.resize(P); desc.resize(8 * P); n_obs.resize(P);
        set.resize((P + 63) / 64, 0);
    }
    void unset_all(size_t P) {
        *this = Store();
        resize(P);
    }
    sivo::LtAttrs view() {
        return sivo::LtAttrs{pos.data(), normal.data(), min_dist.data(), max_dist.data(), desc.data(), n_obs.data()};
    }
    bool is_set(int32_t p) const { return (set[(size_t)p >> 6] >> (p & 63)) & 1u; }
};
inline std::map<sivo_localmap *, Store> &stores() { static std::map<sivo_localmap *, Store> s; return s; }
inline int &map_device() { static int d = 0; return d; }      // what a test sets to stand for a handle on another device
inline long &searches() { static long n = 0; return n; }      // how many sivo_localmap_search_local_points calls were made
inline int refuse(const char *where, const std::string &what) { return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, where, what); }
}  // namespace localmap_track_host

extern "C" {

int sivo_localmap_create(const SivoLocalMapTables *t, sivo_localmap_t *map) {
    const int rc = localmap_base_create(t, map);
    if (rc == SIVO_OK) localmap_track_host::stores()[*map].unset_all((size_t)t->n_points);
    return rc;
}

int sivo_localmap_replace(sivo_localmap_t m, const SivoLocalMapTables *t) {
    const int rc = localmap_base_replace(m, t);
    if (rc == SIVO_OK) localmap_track_host::stores()[m].unset_all((size_t)t->n_points);
    return rc;
}

int sivo_localmap_destroy(sivo_localmap_t m) {
    localmap_track_host::stores().erase(m);
    return localmap_base_destroy(m);
}

int sivo_localmap_apply(sivo_localmap_t m, const SivoLocalMapDelta *dl) {
    const int rc = localmap_base_apply(m, dl);
    if (rc == SIVO_OK && m) localmap_track_host::stores()[m].resize((size_t)m->t.n_points);
    return rc;
}

int sivo_localmap_set_points(sivo_localmap_t m, int n_rows, const int32_t *point_idx, const float *pos, const float *normal,
                             const float *min_dist, const float *max_dist, const uint8_t *desc, const int32_t *n_obs) {
    using namespace localmap_track_host;
    if (!m) return refuse("sivo_localmap_set_points", "null handle");
    const std::string e = sivo::lt_check_set_points(m->t.n_points, n_rows, point_idx, pos, normal, min_dist, max_dist, desc, n_obs);
    if (!e.empty()) return refuse("sivo_localmap_set_points", e);
    if (n_rows == 0) return SIVO_OK;
    Store &s = stores()[m];
    std::vector<uint32_t> words(8 * (size_t)n_rows);                // (the caller's bytes need not be aligned to words)
    std::memcpy(words.data(), desc, 32 * (size_t)n_rows);
    sivo::LtRows r;
    r.n = n_rows; r.idx = point_idx; r.pos = const_cast<float *>(pos); r.normal = const_cast<float *>(normal);
    r.min_dist = const_cast<float *>(min_dist); r.max_dist = const_cast<float *>(max_dist); r.desc = words.data();
    r.n_obs = const_cast<int32_t *>(n_obs);
    const sivo::LtAttrs a = s.view();
    for (int32_t j = 0; j < n_rows; ++j) {
        sivo::lt_scatter_row(a, r, j);
        if (!s.is_set(point_idx[j])) { s.set[(size_t)point_idx[j] >> 6] |= (uint64_t)1 << (point_idx[j] & 63); ++s.n_set; }
    }
    return SIVO_OK;
}

int sivo_localmap_get_points(sivo_localmap_t m, int n_rows, const int32_t *point_idx, float *pos, float *normal, float *min_dist,
                             float *max_dist, uint8_t *desc, int32_t *n_obs, uint8_t *is_set) {
    using namespace localmap_track_host;
    if (!m) return refuse("sivo_localmap_get_points", "null handle");
    const std::string e = sivo::lt_check_get_points(m->t.n_points, n_rows, point_idx, pos, normal, min_dist, max_dist, desc, n_obs, is_set);
    if (!e.empty()) return refuse("sivo_localmap_get_points", e);
    if (n_rows == 0) return SIVO_OK;
    Store &s = stores()[m];
    std::vector<uint32_t> words(8 * (size_t)n_rows);
    sivo::LtRows r;
    r.n = n_rows; r.idx = point_idx; r.pos = pos; r.normal = normal; r.min_dist = min_dist; r.max_dist = max_dist; r.desc = words.data();
    r.n_obs = n_obs;
    const sivo::LtAttrs a = s.view();
    for (int32_t j = 0; j < n_rows; ++j) sivo::lt_gather_row(a, r, j);
    std::memcpy(desc, words.data(), 32 * (size_t)n_rows);
    for (int32_t j = 0; j < n_rows; ++j) {
        is_set[j] = s.is_set(point_idx[j]) ? 1 : 0;
        if (is_set[j]) continue;
        std::memset(pos + 3 * (size_t)j, 0, 12); std::memset(normal + 3 * (size_t)j, 0, 12); std::memset(desc + 32 * (size_t)j, 0, 32);
        min_dist[j] = 0.0f; max_dist[j] = 0.0f; n_obs[j] = 0;
    }
    return SIVO_OK;
}

int sivo_localmap_search_local_points(sivo_localmap_t m, sivo_mframe_t F, const SivoFrustum *frustum, int n_slots, const int32_t *frame_point,
                                      int n_kf_premarked, const int32_t *kf_premarked, int n_point_premarked, const int32_t *point_premarked,
                                      int n_prev, const int32_t *prev_local_kf, int n_seen, const int32_t *seen_point, float th, float nn_ratio,
                                      int32_t *voted, uint8_t *slot_cleared, int kf_capacity, int32_t *local_kf, int32_t *n_local_kf,
                                      int32_t *ref_kf, int point_capacity, int32_t *local_point, int32_t *n_local_points, int32_t *counts,
                                      uint8_t *status, float *proj_x, float *proj_y, float *proj_xr, float *view_cos, int32_t *level,
                                      int32_t *match, int *n_to_match, int *n_matches) {
    using namespace localmap_track_host;
    using namespace sivo;
    const char *who = "sivo_localmap_search_local_points";
    ++searches();
    if (!m) return refuse(who, "null handle");
    if (!F) return refuse(who, "null frame");
    int64_t g_prev = 0;
    if (const char *e = lm_check_update(m->t.n_kf, m->t.n_points, m->t.slot_off, n_slots, frame_point, n_kf_premarked, kf_premarked,
                                        n_point_premarked, point_premarked, n_prev, prev_local_kf, voted, slot_cleared, kf_capacity, local_kf,
                                        n_local_kf, ref_kf, point_capacity, local_point, n_local_points, &g_prev))
        return refuse(who, e);
    Store &s = stores()[m];
    const int nk = (int)F->keys.size();
    const std::string e = lt_check_search(map_device(), 0, nk, F->nlevels, frustum, n_slots, m->t.n_points, s.set.data(), s.n_set, n_seen,
                                          seen_point, point_capacity, status, match);
    if (!e.empty()) return refuse(who, e);
    LtProduce a;
    fr_camera(*frustum, a.cam);
    // the update, as the library runs it
    const int rc = sivo_localmap_update(m, n_slots, frame_point, n_kf_premarked, kf_premarked, n_point_premarked, point_premarked, n_prev,
                                        prev_local_kf, voted, slot_cleared, kf_capacity, local_kf, n_local_kf, ref_kf, point_capacity, local_point,
                                        n_local_points, counts);
    if (rc != SIVO_OK) {                                            // SIVO_ERR_CAPACITY: the text under this entry point's name
        std::string &msg = localmap_host::error();
        const size_t colon = msg.find(": ");
        if (colon != std::string::npos) msg = std::string(who) + msg.substr(colon);
        return rc;
    }
    const int32_t np = *n_local_points;
    // the skip mark kernel: first[] of a local point is not LM_FIRST_PREMARKED when the point passes are done
    std::vector<uint32_t> first((size_t)m->t.n_points + 1, 1u);
    for (int32_t item = 0; item < n_slots + n_seen; ++item) lt_mark_skip(first.data(), n_slots, frame_point, slot_cleared, n_seen, seen_point, item);
    // the producer kernel
    std::vector<SivoSearchQuery> q((size_t)np + 1);
    std::vector<uint32_t> qdesc(8 * (size_t)np + 8);
    std::vector<uint8_t> blocked((size_t)nk + 1, 0), st((size_t)np + 1);
    std::vector<float> px((size_t)np + 1), py((size_t)np + 1), pxr((size_t)np + 1), vc((size_t)np + 1);
    std::vector<int32_t> lv((size_t)np + 1);
    a.th = th; a.n = np; a.local_point = local_point; a.first = first.data(); a.at = s.view(); a.scale = F->scale.data();
    a.q = q.data(); a.qdesc = qdesc.data(); a.status = st.data(); a.px = px.data(); a.py = py.data(); a.pxr = pxr.data(); a.vc = vc.data();
    a.level = lv.data(); a.n_keys = nk; a.frame_point = frame_point; a.slot_cleared = slot_cleared; a.blocked = blocked.data();
    for (int32_t i = 0; i < np; ++i) lt_produce_point(a, i);
    for (int32_t k = 0; k < nk; ++k) blocked[(size_t)k] = lt_blocked(frame_point, slot_cleared, a.at.n_obs, k);
    // the engine: SearchByProjection in sequence over the queries (ORBmatcher.cc:79-123)
    for (int k = 0; k < nk; ++k) match[k] = -1;
    int to_match = 0, nmatches = 0;
    std::vector<int> cand;
    for (int32_t i = 0; i < np; ++i) {
        status[i] = st[(size_t)i];
        if (st[(size_t)i] != SIVO_FRUSTUM_IN_VIEW) continue;
        ++to_match;
        if (proj_x) proj_x[i] = px[(size_t)i];
        if (proj_y) proj_y[i] = py[(size_t)i];
        if (proj_xr) proj_xr[i] = pxr[(size_t)i];
        if (view_cos) view_cos[i] = vc[(size_t)i];
        if (level) level[i] = lv[(size_t)i];
        const SivoSearchQuery &Q = q[(size_t)i];
        frustum_host::features_in_area(*F, Q.u, Q.v, Q.radius, Q.lvl_lo, Q.lvl_hi, cand);
        int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
        for (int idx : cand) {
            if (blocked[(size_t)idx]) continue;
            if (F->u_right[(size_t)idx] > 0) {
                const float er = std::fabs(Q.ur - F->u_right[(size_t)idx]);
                if (er > Q.gate) continue;
            }
            const int dist = frustum_host::distance((const uint8_t *)(qdesc.data() + 8 * (size_t)i), F->desc.data() + 32 * (size_t)idx);
            if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = F->keys[(size_t)idx].octave; bestIdx = idx; }
            else if (dist < bestDist2) { bestLevel2 = F->keys[(size_t)idx].octave; bestDist2 = dist; }
        }
        if (bestDist <= 100) {
            if (bestLevel == bestLevel2 && (float)bestDist > nn_ratio * (float)bestDist2) continue;
            match[bestIdx] = i;
            blocked[(size_t)bestIdx] = Q.flags & SIVO_Q_BLOCKS ? 1 : 0;
            ++nmatches;
        }
    }
    if (n_to_match) *n_to_match = to_match;
    if (n_matches) *n_matches = nmatches;
    return SIVO_OK;
}

}  // extern "C"
