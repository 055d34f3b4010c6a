// covis_math.hpp — the per-slot bodies of the covisibility bookkeeping: the counting loop of KeyFrame::UpdateConnections (reference
// src/orbslam/KeyFrame.cc:340-360) and Tracking::UpdateLocalKeyFrames (Tracking.cc:1129-1142), one slot of LocalMapping::KeyFrameCulling
// (LocalMapping.cc:745-786) with what KeyFrame::SetBadFlag -> MapPoint::EraseObservation (KeyFrame.cc:493-495, MapPoint.cc:164-189) leaves
// behind, and one point of LocalMapping::MapPointCulling (LocalMapping.cc:181-194); shared by the kernels (covis.hip) and, compiled by
// g++, by the host programs of the tests.  Integers throughout, except the depth rule, the found ratio and the 0.9 comparison.
//
// Keyframe culling keeps the reference's sequential state in two byte arrays: removed[k] (keyframe k was culled and was erasable: its
// observations have left every point) and bad[p] (isBad() as it stands now).  What the reference reads from a point is derived from
// the table and those: mObservations is the list without the removed keyframes, nObs the weighted sum over that list.
#pragma once
#include <stdint.h>

#include "../../include/sivo_hip.h"

#ifndef SIVO_HD
#ifdef __HIPCC__
#define SIVO_HD __host__ __device__ inline
#else
#define SIVO_HD inline
#endif
#endif

namespace sivo {

// The slot of a set: `add(k)` for every observer k of the point but `self` (KeyFrame.cc:346-359; self = -1 skips none)
template <class Add>
SIVO_HD void cv_count_slot(const SivoObsTable &t, int32_t p, int32_t self, Add &&add) {
    if (p < 0) return;                                                  // (:346)
    if (t.point_bad[p]) return;                                         // (:349)
    for (int64_t o = t.obs_off[p], e = t.obs_off[p + 1]; o < e; ++o) {
        const int32_t k = t.obs_kf[o];
        if (k == self) continue;                                        // (:356)
        add(k);
    }
}

struct CvSlot {
    int32_t counted;       // nMPs++ (LocalMapping.cc:756)
    int32_t redundant;     // nRedundantObservations++ (:782)
    int32_t goes_bad;      // were the keyframe culled now, EraseObservation would leave the point with nObs <= 2 (MapPoint.cc:181)
};

// Slot (p, level, depth) of keyframe kf.  `counted` and `redundant` are the loop body of :746-785; goes_bad concerns every slot that holds
// a point (KeyFrame.cc:493-495 walks them all, the depth rule plays no part there).
SIVO_HD CvSlot cv_kf_slot(const SivoObsTable &t, const uint8_t *bad, const uint8_t *removed, int32_t kf, int32_t p, int32_t level, float depth,
                          float th_depth, int monocular) {
    CvSlot r = {0, 0, 0};
    if (p < 0) return r;                                                // (:747)
    if (bad[p]) return r;                                               // (:748; a bad point's mObservations is empty, MapPoint.cc:208)
    int32_t n_obs = 0, w_self = 0, others = 0;
    bool lists_self = false;
    for (int64_t o = t.obs_off[p], e = t.obs_off[p + 1]; o < e; ++o) {
        const int32_t k = t.obs_kf[o];
        if (removed[k]) continue;                                       // erased from mObservations by an earlier SetBadFlag
        const int32_t w = t.obs_stereo[o] ? 2 : 1;                      // (MapPoint.cc:157-161)
        n_obs += w;
        if (k == kf) {                                                  // (:767)
            lists_self = true;
            w_self += w;
            continue;
        }
        if ((int32_t)t.obs_level[o] <= level + 1) ++others;             // (:774; the break of :777 does not change nObs >= thObs)
    }
    r.goes_bad = lists_self && n_obs - w_self <= 2;                     // (MapPoint.cc:168-182)
    if (!monocular && (depth > th_depth || depth < 0.0f)) return r;     // (:749-753: a NaN is neither)
    r.counted = 1;
    r.redundant = n_obs > 3 && others >= 3;                             // (:757, :781)
    return r;
}

// (:789) with KeyFrame::SetBadFlag's two early returns (KeyFrame.cc:480-485)
SIVO_HD uint8_t cv_kf_decision(int32_t n_redundant, int32_t n_mps, int erasable) {
    if (!((double)n_redundant > 0.9 * (double)n_mps)) return SIVO_KFCULL_KEPT;
    return erasable ? SIVO_KFCULL_CULLED : SIVO_KFCULL_TO_BE_ERASED;
}

// One point of LocalMapping::MapPointCulling (:181-194)
SIVO_HD uint8_t cv_mappoint_status(int32_t found, int32_t visible, int64_t first_kf_id, int32_t n_obs, uint8_t bad, int64_t current_kf_id,
                                   int monocular) {
    if (bad) return SIVO_MPCULL_ALREADY_BAD;
    if ((float)found / (float)visible < 0.25f) return SIVO_MPCULL_FOUND_RATIO;      // (MapPoint.cc:281: 0 / 0 and 1 / 0 are not below)
    // ((int) nCurrentKFid - (int) pMP->mnFirstKFid): both truncated to 32 bits, the difference taken there
    const int32_t age = (int32_t)((uint32_t)(uint64_t)current_kf_id - (uint32_t)(uint64_t)first_kf_id);
    if (age >= 2 && n_obs <= (monocular ? 2 : 3)) return SIVO_MPCULL_OBSERVATIONS;
    if (age >= 3) return SIVO_MPCULL_AGED_OUT;
    return SIVO_MPCULL_STAYS;
}

// ---- argument checks, host only: the text of what is wrong, or nullptr -------------------------------------------------------------
inline const char *cv_check_csr(const int64_t *off, int64_t n, const char *null_text, const char *start_text, const char *order_text) {
    if (n < 0) return "negative count";
    if (n == 0) return nullptr;
    if (!off) return null_text;
    if (off[0] != 0) return start_text;
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return order_text;
    if (off[n] > ((int64_t)1 << 28)) return "more than 2^28 entries";
    return nullptr;
}

inline const char *cv_check_table(const SivoObsTable *t) {
    if (!t) return "null table";
    if (t->n_kf < 0 || t->n_points < 0) return "negative count";
    if (t->n_kf > (1 << 24) || t->n_points > (1 << 24)) return "more than 2^24 keyframes or points";
    if (const char *e = cv_check_csr(t->obs_off, t->n_points, "null obs_off", "obs_off does not start at 0", "obs_off decreases")) return e;
    if (t->n_points == 0) return nullptr;
    if (!t->point_bad) return "null point_bad";
    const int64_t n = t->obs_off[t->n_points];
    if (n && (!t->obs_kf || !t->obs_level || !t->obs_stereo)) return "null observation array";
    for (int64_t o = 0; o < n; ++o)
        if (t->obs_kf[o] < 0 || t->obs_kf[o] >= t->n_kf) return "obs_kf outside 0 .. n_kf - 1";
    return nullptr;
}

// -1 .. n - 1 (lo = -1) or 0 .. n - 1 (lo = 0)
inline const char *cv_check_index(const int32_t *idx, int64_t count, int32_t lo, int32_t n, const char *null_text, const char *range_text) {
    if (count == 0) return nullptr;
    if (!idx) return null_text;
    for (int64_t i = 0; i < count; ++i)
        if (idx[i] < lo || idx[i] >= n) return range_text;
    return nullptr;
}

inline const char *cv_check_count(const SivoObsTable *t, int n_sets, const int64_t *set_off, const int32_t *set_point, const int32_t *set_self,
                                  const int32_t *counts) {
    if (const char *e = cv_check_table(t)) return e;
    if (const char *e = cv_check_csr(set_off, n_sets, "null set_off", "set_off does not start at 0", "set_off decreases")) return e;
    if (n_sets == 0) return nullptr;
    if (const char *e = cv_check_index(set_point, set_off[n_sets], -1, t->n_points, "null set_point", "set_point outside -1 .. n_points - 1")) return e;
    if (const char *e = cv_check_index(set_self, n_sets, -1, t->n_kf, "null set_self", "set_self outside -1 .. n_kf - 1")) return e;
    if ((int64_t)n_sets * t->n_kf > ((int64_t)1 << 28)) return "more than 2^28 counters";
    if (t->n_kf && !counts) return "null counts";
    return nullptr;
}

inline const char *cv_check_kfcull(const SivoObsTable *t, int n_local, const int32_t *local_kf, const uint8_t *is_id0, const uint8_t *erasable,
                                   const float *th_depth, const int64_t *slot_off, const int32_t *slot_point, const uint8_t *slot_level,
                                   const float *slot_depth, const int32_t *n_mps, const int32_t *n_redundant, const uint8_t *decision,
                                   const uint8_t *bad_after) {
    if (const char *e = cv_check_table(t)) return e;
    if (t->n_points && !bad_after) return "null bad_after";
    if (const char *e = cv_check_csr(slot_off, n_local, "null slot_off", "slot_off does not start at 0", "slot_off decreases")) return e;
    if (n_local == 0) return nullptr;
    if (!is_id0 || !erasable || !th_depth || !n_mps || !n_redundant || !decision) return "null keyframe array";
    if (const char *e = cv_check_index(local_kf, n_local, 0, t->n_kf, "null local_kf", "local_kf outside 0 .. n_kf - 1")) return e;
    if (slot_off[n_local] && (!slot_level || !slot_depth)) return "null slot array";
    return cv_check_index(slot_point, slot_off[n_local], -1, t->n_points, "null slot_point", "slot_point outside -1 .. n_points - 1");
}

inline const char *cv_check_mpcull(int n, const int32_t *found, const int32_t *visible, const int64_t *first_kf_id, const int32_t *n_obs,
                                   const uint8_t *bad, const uint8_t *status) {
    if (n < 0) return "negative count";
    if (n > (1 << 24)) return "more than 2^24 points";
    if (n && (!found || !visible || !first_kf_id || !n_obs || !bad || !status)) return "null array";
    return nullptr;
}

}  // namespace sivo
