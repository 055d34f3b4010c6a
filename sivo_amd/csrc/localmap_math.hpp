// localmap_math.hpp — the per-item bodies of Tracking::UpdateLocalMap on arrays (reference src/orbslam/Tracking.cc:1096-1235): what a frame
// slot, a keyframe of the vote, a neighbour candidate and a slot of a local keyframe each decide, and the argument checks of the
// sivo_localmap_* entry points; shared by the kernels (localmap.hip) and, compiled by g++, by the host programs of the tests
// (tests/localmap_host_capi.hpp).  Integers throughout.
//
// The point passes see the slots of all local keyframes as one sequence g = 0 .. G - 1 (keyframe order, then slot order; list_off is the
// exclusive prefix over the keyframes' slot counts).  first[p] holds g + 1 of the first slot that holds point p: LM_FIRST_NONE where no
// slot does, LM_FIRST_PREMARKED (0, below every g + 1) where mnTrackReferenceForFrame already equals the frame's id.
#pragma once
#include <stdint.h>

#include <vector>

#include "covis_math.hpp"

namespace sivo {

constexpr int LM_MAX_LOCAL = 80;                     // (:1183)
constexpr int LM_BEST_COVIS = 10;                    // (:1189)
constexpr uint32_t LM_FIRST_NONE = 0xFFFFFFFFu;
constexpr uint32_t LM_FIRST_PREMARKED = 0u;

// the part of the tables the vote reads, for cv_count_slot
SIVO_HD SivoObsTable lm_obs_table(const SivoLocalMapTables &t) {
    SivoObsTable o;
    o.n_kf = t.n_kf; o.n_points = t.n_points; o.obs_off = t.obs_off; o.obs_kf = t.obs_kf; o.obs_level = nullptr; o.obs_stereo = nullptr;
    o.point_bad = t.point_bad;
    return o;
}

// mCurrentFrame.mvpMapPoints[i] = nullptr (:1138-1140)
SIVO_HD uint8_t lm_slot_cleared(const SivoLocalMapTables &t, int32_t p) { return p >= 0 && t.point_bad[p] ? 1 : 0; }

// keyframe k is in keyframeCounter and passes :1162
SIVO_HD bool lm_stage1_takes(const SivoLocalMapTables &t, const int32_t *counts, int32_t k) { return counts[k] > 0 && !t.kf_bad[k]; }

// (count, position in the walk) as one key whose maximum is the first strict maximum of :1165-1168; 0 = nobody
SIVO_HD uint64_t lm_max_key(int32_t count, int32_t pos) { return ((uint64_t)(uint32_t)count << 32) | (uint32_t)(0x7FFFFFFF - pos); }
SIVO_HD int32_t lm_key_pos(uint64_t key) { return 0x7FFFFFFF - (int32_t)(uint32_t)key; }

// mnTrackReferenceForFrame == mCurrentFrame.mnId of keyframe k, one bit each
SIVO_HD bool lm_marked(const uint32_t *marks, int32_t k) { return (marks[k >> 5] >> (k & 31)) & 1u; }
SIVO_HD uint32_t lm_mark_bit(int32_t k) { return 1u << (k & 31); }

// a covisible or a child that stage 2 takes (:1197-1198, :1212-1213)
SIVO_HD bool lm_neighbour_ok(const SivoLocalMapTables &t, const uint32_t *marks, int32_t c) { return !t.kf_bad[c] && !lm_marked(marks, c); }

// the i with list_off[i] <= g < list_off[i + 1] (keyframes without slots are stepped over), n >= 1, 0 <= g < list_off[n]
SIVO_HD int32_t lm_find_kf(const int32_t *list_off, int32_t n, int32_t g) {
    int32_t lo = 0, hi = n;                          // list_off[lo] <= g < list_off[hi]
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (list_off[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the point in slot g of the sequence (:1105-1108), -1 for a null slot
SIVO_HD int32_t lm_slot_point(const SivoLocalMapTables &t, const int32_t *list, const int32_t *list_off, int32_t n, int32_t g) {
    const int32_t i = lm_find_kf(list_off, n, g);
    return t.slot_point[t.slot_off[list[i]] + (g - list_off[i])];
}

// slot g pushes its point (:1110-1121): not null, the first slot that holds it, not marked before the call, and — tested last — not bad
SIVO_HD bool lm_point_survives(const SivoLocalMapTables &t, const uint32_t *first, int32_t p, int32_t g) {
    return p >= 0 && first[p] == (uint32_t)g + 1u && !t.point_bad[p];
}

// ---- argument checks, host only: the text of what is wrong, or nullptr -------------------------------------------------------------
inline const char *lm_check_tables(const SivoLocalMapTables *t) {
    if (!t) return "null tables";
    if (t->n_kf < 0 || t->n_points < 0) return "negative count";
    if (t->n_kf > (1 << 24) || t->n_points > (1 << 24)) return "more than 2^24 keyframes or points";
    const int32_t K = t->n_kf, P = t->n_points;
    if (const char *e = cv_check_csr(t->obs_off, P, "null obs_off", "obs_off does not start at 0", "obs_off decreases")) return e;
    if (P) {
        if (!t->point_bad) return "null point_bad";
        if (const char *e = cv_check_index(t->obs_kf, t->obs_off[P], 0, K, "null obs_kf", "obs_kf outside 0 .. n_kf - 1")) return e;
    }
    if (K == 0) return nullptr;
    if (!t->kf_bad) return "null kf_bad";
    if (const char *e = cv_check_csr(t->slot_off, K, "null slot_off", "slot_off does not start at 0", "slot_off decreases")) return e;
    if (const char *e = cv_check_index(t->slot_point, t->slot_off[K], -1, P, "null slot_point", "slot_point outside -1 .. n_points - 1")) return e;
    if (const char *e = cv_check_csr(t->covis_off, K, "null covis_off", "covis_off does not start at 0", "covis_off decreases")) return e;
    if (const char *e = cv_check_index(t->covis_kf, t->covis_off[K], 0, K, "null covis_kf", "covis_kf outside 0 .. n_kf - 1")) return e;
    if (const char *e = cv_check_csr(t->child_off, K, "null child_off", "child_off does not start at 0", "child_off decreases")) return e;
    if (const char *e = cv_check_index(t->child_kf, t->child_off[K], 0, K, "null child_kf", "child_kf outside 0 .. n_kf - 1")) return e;
    if (const char *e = cv_check_index(t->parent, K, -1, K, "null parent", "parent outside -1 .. n_kf - 1")) return e;
    if (t->kf_order) {
        std::vector<uint8_t> seen((size_t)K, 0);
        for (int32_t i = 0; i < K; ++i) {
            const int32_t k = t->kf_order[i];
            if (k < 0 || k >= K || seen[(size_t)k]) return "kf_order is not a permutation of 0 .. n_kf - 1";
            seen[(size_t)k] = 1;
        }
    }
    return nullptr;
}

inline const char *lm_check_set_bad(int32_t n_kf_map, int32_t n_points_map, int n_points, const int32_t *point_idx, const uint8_t *point_val, int n_kf,
                                    const int32_t *kf_idx, const uint8_t *kf_val) {
    if (n_points < 0 || n_kf < 0) return "negative count";
    if (const char *e = cv_check_index(point_idx, n_points, 0, n_points_map, "null point_idx", "point_idx outside 0 .. n_points - 1")) return e;
    if (n_points && !point_val) return "null point_val";
    if (const char *e = cv_check_index(kf_idx, n_kf, 0, n_kf_map, "null kf_idx", "kf_idx outside 0 .. n_kf - 1")) return e;
    if (n_kf && !kf_val) return "null kf_val";
    return nullptr;
}

// slot_off: the handle's host copy (n_kf_map + 1).  *g_prev receives the slot count of prev_local_kf.
inline const char *lm_check_update(int32_t n_kf_map, int32_t n_points_map, const int64_t *slot_off, int n_slots, const int32_t *frame_point,
                                   int n_kf_premarked, const int32_t *kf_premarked, int n_point_premarked, const int32_t *point_premarked, int n_prev,
                                   const int32_t *prev_local_kf, const int32_t *voted, const uint8_t *slot_cleared, int kf_capacity,
                                   const int32_t *local_kf, const int32_t *n_local_kf, const int32_t *ref_kf, int point_capacity,
                                   const int32_t *local_point, const int32_t *n_local_points, int64_t *g_prev) {
    if (n_slots < 0 || n_kf_premarked < 0 || n_point_premarked < 0 || n_prev < 0 || kf_capacity < 0 || point_capacity < 0) return "negative count";
    if (n_slots > (1 << 24) || n_prev > (1 << 24)) return "more than 2^24 frame slots or previous keyframes";
    if (const char *e = cv_check_index(frame_point, n_slots, -1, n_points_map, "null frame_point", "frame_point outside -1 .. n_points - 1")) return e;
    if (const char *e = cv_check_index(kf_premarked, n_kf_premarked, 0, n_kf_map, "null kf_premarked", "kf_premarked outside 0 .. n_kf - 1")) return e;
    if (const char *e = cv_check_index(point_premarked, n_point_premarked, 0, n_points_map, "null point_premarked", "point_premarked outside 0 .. n_points - 1")) return e;
    if (const char *e = cv_check_index(prev_local_kf, n_prev, 0, n_kf_map, "null prev_local_kf", "prev_local_kf outside 0 .. n_kf - 1")) return e;
    if (!voted || !n_local_kf || !ref_kf || !n_local_points) return "null result";
    if (n_slots && !slot_cleared) return "null slot_cleared";
    if (kf_capacity && !local_kf) return "null local_kf";
    if (point_capacity && !local_point) return "null local_point";
    int64_t g = 0;
    for (int i = 0; i < n_prev; ++i) {
        g += slot_off[prev_local_kf[i] + 1] - slot_off[prev_local_kf[i]];
        if (g > ((int64_t)1 << 28)) return "prev_local_kf holds more than 2^28 slots";
    }
    *g_prev = g;
    return nullptr;
}

}  // namespace sivo
