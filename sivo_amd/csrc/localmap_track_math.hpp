// localmap_track_math.hpp — the per-item bodies of the resident attribute store (sivo_localmap_set_points / _get_points) and of
// sivo_localmap_search_local_points: Tracking::SearchLocalPoints (reference src/orbslam/Tracking.cc:1033-1085) on the mvpLocalMapPoints
// that Tracking::UpdateLocalMap (:1087-1124) has just left on the device.  The row scatter and gather, the skip mark, the attribute
// gather in front of Frame::isInFrustum (fr_point / fr_query / fr_no_query of frustum_math.hpp, unchanged) and the rule of the blocked
// keypoints; shared by the kernels (localmap_track.hip) and, compiled by g++, by the host programs of the tests
// (tests/localmap_track_host_capi.hpp).
//
// The skip mark lives in the update's first[]: after the point passes first[p] of a local point is the position of its first slot
// plus one, never LM_FIRST_PREMARKED (a premarked point does not reach local_point), so that value marks "skip" without a second array
// and without a memset; the next update clears first[] as it always does.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "frustum_math.hpp"
#include "localmap_math.hpp"

namespace sivo {

constexpr size_t LT_ROW_BYTES = 68;        // pos 12, normal 12, min_dist 4, max_dist 4, desc 32, n_obs 4

struct LtAttrs {                           // structure-of-arrays over the handle's point indices
    float *pos, *normal;                   // 3 per point: mWorldPos, mNormalVector
    float *min_dist, *max_dist;            // mfMinDistance, mfMaxDistance raw
    uint32_t *desc;                        // 8 words per point: mDescriptor
    int32_t *n_obs;                        // Observations()
};

struct LtRows {                            // rows in the caller's order (set_points: the upload; get_points: the download)
    int32_t n;
    const int32_t *idx;
    float *pos, *normal, *min_dist, *max_dist;
    uint32_t *desc;
    int32_t *n_obs;
};

// row j of the upload into the store
SIVO_HD void lt_scatter_row(const LtAttrs &a, const LtRows &r, int32_t j) {
    const int64_t p = r.idx[j];
    for (int c = 0; c < 3; ++c) { a.pos[3 * p + c] = r.pos[3 * (int64_t)j + c]; a.normal[3 * p + c] = r.normal[3 * (int64_t)j + c]; }
    a.min_dist[p] = r.min_dist[j]; a.max_dist[p] = r.max_dist[j]; a.n_obs[p] = r.n_obs[j];
    for (int w = 0; w < 8; ++w) a.desc[8 * p + w] = r.desc[8 * (int64_t)j + w];
}

// row j of the download out of the store
SIVO_HD void lt_gather_row(const LtAttrs &a, const LtRows &r, int32_t j) {
    const int64_t p = r.idx[j];
    for (int c = 0; c < 3; ++c) { r.pos[3 * (int64_t)j + c] = a.pos[3 * p + c]; r.normal[3 * (int64_t)j + c] = a.normal[3 * p + c]; }
    r.min_dist[j] = a.min_dist[p]; r.max_dist[j] = a.max_dist[p]; r.n_obs[j] = a.n_obs[p];
    for (int w = 0; w < 8; ++w) r.desc[8 * (int64_t)j + w] = a.desc[8 * p + w];
}

// ---- the skip set: mnLastFrameSeen == mCurrentFrame.mnId when the second loop of SearchLocalPoints reaches the point (:1057) ----------
// item s < n_slots: the frame's own point in slot s, stamped by the first loop (:1035-1049) unless the update cleared the slot;
// item n_slots + j: seen_point[j], stamped before the call (the outliers of :626-630 among them)
SIVO_HD void lt_mark_skip(uint32_t *first, int32_t n_slots, const int32_t *frame_point, const uint8_t *slot_cleared, int32_t n_seen,
                          const int32_t *seen_point, int32_t item) {
    if (item < n_slots) {
        const int32_t p = frame_point[item];
        if (p >= 0 && !slot_cleared[item]) first[p] = LM_FIRST_PREMARKED;
    } else if (item - n_slots < n_seen) {
        first[seen_point[item - n_slots]] = LM_FIRST_PREMARKED;
    }
}
SIVO_HD bool lt_skipped(const uint32_t *first, int32_t p) { return first[p] == LM_FIRST_PREMARKED; }

// ---- the producer: local point i and keypoint k ------------------------------------------------------------------------------------
struct LtProduce {
    FrCamera cam;
    float th;
    int32_t n;                             // local points
    const int32_t *local_point;
    const uint32_t *first;                 // the skip marks
    LtAttrs at;
    const float *scale;                    // the frame's mvScaleFactors
    SivoSearchQuery *q;                    // n records
    uint32_t *qdesc;                       // 8 words per record
    uint8_t *status;
    float *px, *py, *pxr, *vc;             // written for the points in view only
    int32_t *level;
    int32_t n_keys;                        // the frame's keypoints == the update's n_slots
    const int32_t *frame_point;
    const uint8_t *slot_cleared;
    uint8_t *blocked;
};

// The second loop of SearchLocalPoints (:1054-1070) for local point i and the query ORBmatcher::SearchByProjection makes of it
// (ORBmatcher.cc:57-76): what fr_queries_kernel of search.hip does on arrays the host gathered, here on local_point[i]'s stored row.
SIVO_HD void lt_produce_point(const LtProduce &a, int32_t i) {
    const int64_t p = a.local_point[i];
    uint8_t st = SIVO_FRUSTUM_SKIPPED;
    FrResult o;
    if (!lt_skipped(a.first, (int32_t)p)) {
        const float X[3] = {a.at.pos[3 * p], a.at.pos[3 * p + 1], a.at.pos[3 * p + 2]};
        const float N[3] = {a.at.normal[3 * p], a.at.normal[3 * p + 1], a.at.normal[3 * p + 2]};
        st = fr_point(a.cam, X, N, a.at.min_dist[p], a.at.max_dist[p], o);
    }
    SivoSearchQuery q;
    if (st == SIVO_FRUSTUM_IN_VIEW) {
        fr_query(o, a.th, a.scale, a.at.n_obs[p], q);
        a.px[i] = o.u; a.py[i] = o.v; a.pxr[i] = o.ur; a.vc[i] = o.view_cos; a.level[i] = o.level;
    } else {
        fr_no_query(q);
    }
    a.q[i] = q;
    a.status[i] = st;
    for (int w = 0; w < 8; ++w) a.qdesc[8 * (int64_t)i + w] = a.at.desc[8 * p + w];
}

// occ_obs[k] > 0 of sivo_search_local_points: the keypoint holds a point (its slot was not cleared) with Observations() > 0
// (ORBmatcher.cc:88-90)
SIVO_HD uint8_t lt_blocked(const int32_t *frame_point, const uint8_t *slot_cleared, const int32_t *n_obs, int32_t k) {
    const int32_t p = frame_point[k];
    return p >= 0 && !slot_cleared[k] && n_obs[p] > 0 ? 1 : 0;
}

// ---- argument checks, host only: the text of what is wrong, or an empty string -----------------------------------------------------
inline std::string lt_check_rows(int32_t n_points_map, int n_rows, const int32_t *point_idx, bool arrays_present, const char *null_text) {
    if (n_rows < 0) return "negative count";
    if (n_rows == 0) return "";
    if (!point_idx) return "null point_idx";
    if (!arrays_present) return null_text;
    for (int i = 0; i < n_rows; ++i) {
        if (point_idx[i] < 0 || point_idx[i] >= n_points_map) return "point_idx outside 0 .. n_points - 1";
        if (i && point_idx[i] <= point_idx[i - 1]) return "point_idx is not strictly increasing";
    }
    return "";
}

inline std::string lt_check_set_points(int32_t n_points_map, int n_rows, const int32_t *point_idx, const float *pos, const float *normal,
                                       const float *min_dist, const float *max_dist, const uint8_t *desc, const int32_t *n_obs) {
    return lt_check_rows(n_points_map, n_rows, point_idx, pos && normal && min_dist && max_dist && desc && n_obs, "null attribute array");
}

inline std::string lt_check_get_points(int32_t n_points_map, int n_rows, const int32_t *point_idx, const float *pos, const float *normal,
                                       const float *min_dist, const float *max_dist, const uint8_t *desc, const int32_t *n_obs,
                                       const uint8_t *is_set) {
    return lt_check_rows(n_points_map, n_rows, point_idx, pos && normal && min_dist && max_dist && desc && n_obs && is_set, "null output array");
}

// what sivo_localmap_search_local_points refuses beyond sivo_localmap_update's own checks.  attr_set: the handle's bitmap.
inline std::string lt_check_search(int map_device, int frame_device, int frame_keys, int frame_levels, const SivoFrustum *frustum, int n_slots,
                                   int32_t n_points_map, const uint64_t *attr_set, int64_t n_attr_set, int n_seen, const int32_t *seen_point,
                                   int point_capacity, const uint8_t *status, const int32_t *match) {
    if (!frustum) return "null frustum";
    if (map_device != frame_device) {
        char text[96];
        snprintf(text, sizeof text, "the map is on device %d and the frame on device %d", map_device, frame_device);
        return text;
    }
    if (n_slots != frame_keys) {
        char text[96];
        snprintf(text, sizeof text, "n_slots is %d and the frame has %d keypoints", n_slots, frame_keys);
        return text;
    }
    if (frustum->nlevels < 1 || frustum->nlevels > 16) return "nlevels outside 1 .. 16";
    if (frustum->nlevels > frame_levels) return "the frustum has more levels than the frame's scale tables";
    if (!(frustum->log_scale_factor > 0.0f)) return "log_scale_factor must be positive";
    if (n_seen < 0) return "negative count";
    if (const char *e = cv_check_index(seen_point, n_seen, 0, n_points_map, "null seen_point", "seen_point outside 0 .. n_points - 1")) return e;
    if (point_capacity && !status) return "null status";
    if (frame_keys && !match) return "null match";
    if (n_attr_set != n_points_map) {
        int32_t first = -1;
        for (int32_t p = 0; p < n_points_map && first < 0; ++p)
            if (!((attr_set[(size_t)p >> 6] >> (p & 63)) & 1u)) first = p;
        char text[128];
        snprintf(text, sizeof text, "%lld of the handle's %d points have no attributes, the first is point %d", (long long)(n_points_map - n_attr_set),
                 (int)n_points_map, (int)first);
        return text;
    }
    return "";
}

}  // namespace sivo
