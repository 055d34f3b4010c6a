// ba_window_math.hpp — the per-item bodies of the window of Optimizer::LocalBundleAdjustment on arrays (reference
// src/orbslam/Optimizer.cc:496-559, :585-622, :651-670): what a candidate, an observation of a local point and a slot of an observer each
// decide, and the argument check of sivo_localmap_ba_window; shared by the kernels (ba_window.hip) and, compiled by g++, by the host
// programs of the tests (tests/ba_window_host_capi.hpp).  Integers throughout.
//
// The fixed-keyframe passes see the observation rows of all local points as one sequence h = 0 .. H - 1 (point order, then row order;
// row_off is the exclusive prefix over the points' row lengths).  kf_first[k] holds h + 1 of the first observation by keyframe k:
// BW_FIRST_NONE where nobody observes, BW_FIRST_MARKED (0, below every h + 1) where mnBALocalForKF or mnBAFixedForKF already equals
// pKF->mnId when the walk of :538 begins.  pose_of[k] is the vertex of keyframe k (:585-622), -1 where it has none.
#pragma once
#include <stdint.h>

#include <vector>

#include "localmap_math.hpp"

namespace sivo {

constexpr uint32_t BW_FIRST_NONE = 0xFFFFFFFFu;
constexpr uint32_t BW_FIRST_MARKED = 0u;

// candidate i becomes a local keyframe: pKF unconditionally (:499), a covisible where it is not bad (:510-512)
SIVO_HD bool bw_cand_listed(const SivoLocalMapTables &t, const int32_t *cand, int32_t i) { return i == 0 || !t.kf_bad[cand[i]]; }

// the observations of local point i
SIVO_HD int32_t bw_row_len(const SivoLocalMapTables &t, const int32_t *local_point, int32_t i) {
    return (int32_t)(t.obs_off[local_point[i] + 1] - t.obs_off[local_point[i]]);
}

// observation h of the sequence: local point i (point p), entry r of its row, keyframe k.  n >= 1, 0 <= h < row_off[n]
struct BwObs {
    int32_t i, r, p, k;
};
SIVO_HD BwObs bw_obs(const SivoLocalMapTables &t, const int32_t *local_point, const int32_t *row_off, int32_t n, int32_t h) {
    BwObs o;
    o.i = lm_find_kf(row_off, n, h);
    o.r = h - row_off[o.i];
    o.p = local_point[o.i];
    o.k = t.obs_kf[t.obs_off[o.p] + o.r];
    return o;
}

// observation h pushes its keyframe into lFixedKFs (:551-556): the first that meets it, it was not marked before, and — tested last — not bad
SIVO_HD bool bw_fixed_survives(const SivoLocalMapTables &t, const uint32_t *kf_first, int32_t k, int32_t h) {
    return kf_first[k] == (uint32_t)h + 1u && !t.kf_bad[k];
}

// an observation by keyframe k becomes an edge (:670; a keyframe without a vertex has no edge)
SIVO_HD bool bw_edge_kept(const SivoLocalMapTables &t, const int32_t *pose_of, int32_t k) { return !t.kf_bad[k] && pose_of[k] >= 0; }

// how many of the first `upto` observations of point p become edges
SIVO_HD int32_t bw_kept_before(const SivoLocalMapTables &t, const int32_t *pose_of, int32_t p, int32_t upto) {
    int32_t n = 0;
    for (int64_t o = t.obs_off[p], e = o + upto; o < e; ++o) n += bw_edge_kept(t, pose_of, t.obs_kf[o]) ? 1 : 0;
    return n;
}

// slot s of keyframe k holds point p
SIVO_HD bool bw_slot_hit(const SivoLocalMapTables &t, int32_t k, int32_t s, int32_t p) { return t.slot_point[t.slot_off[k] + s] == p; }

// edge_slot from the number of slots that hold the point and the lowest of them
SIVO_HD int32_t bw_slot_code(int32_t hits, int32_t lowest) {
    return hits == 1 ? lowest : hits == 0 ? SIVO_BAWIN_SLOT_NONE : SIVO_BAWIN_SLOT_AMBIGUOUS;
}

// ---- the argument check, host only: the text of what is wrong, or nullptr ------------------------------------------------------------
inline const char *bw_check_window(int32_t n_kf_map, int32_t n_points_map, int64_t total_slots, int64_t total_obs, int n_cand, const int32_t *cand_kf,
                                   int n_kf_local_pre, const int32_t *kf_local_pre, int n_kf_fixed_pre, const int32_t *kf_fixed_pre, int n_point_pre,
                                   const int32_t *point_pre, int kf_capacity, const int32_t *local_kf, const int32_t *fixed_kf, int point_capacity,
                                   const int32_t *local_point, const int64_t *edge_off, int64_t edge_capacity, const int32_t *edge_pose,
                                   const int32_t *edge_slot, const int64_t *counts) {
    if (n_cand < 0 || n_kf_local_pre < 0 || n_kf_fixed_pre < 0 || n_point_pre < 0 || kf_capacity < 0 || point_capacity < 0 || edge_capacity < 0)
        return "negative count";
    if (n_cand < 1) return "n_cand < 1: cand_kf[0] is the keyframe of the window";
    if (const char *e = cv_check_index(cand_kf, n_cand, 0, n_kf_map, "null cand_kf", "cand_kf outside 0 .. n_kf - 1")) return e;
    {
        std::vector<uint8_t> seen((size_t)n_kf_map, 0);
        for (int i = 0; i < n_cand; ++i) {
            if (seen[(size_t)cand_kf[i]]) return "cand_kf lists a keyframe twice";
            seen[(size_t)cand_kf[i]] = 1;
        }
    }
    if (const char *e = cv_check_index(kf_local_pre, n_kf_local_pre, 0, n_kf_map, "null kf_local_pre", "kf_local_pre outside 0 .. n_kf - 1")) return e;
    if (const char *e = cv_check_index(kf_fixed_pre, n_kf_fixed_pre, 0, n_kf_map, "null kf_fixed_pre", "kf_fixed_pre outside 0 .. n_kf - 1")) return e;
    if (const char *e = cv_check_index(point_pre, n_point_pre, 0, n_points_map, "null point_pre", "point_pre outside 0 .. n_points - 1")) return e;
    if (!counts) return "null counts";
    if (kf_capacity && !local_kf) return "null local_kf";
    if (kf_capacity && !fixed_kf) return "null fixed_kf";
    if (point_capacity && !local_point) return "null local_point";
    if (!edge_off) return "null edge_off";
    if (edge_capacity && !edge_pose) return "null edge_pose";
    if (edge_capacity && !edge_slot) return "null edge_slot";
    if (total_slots > ((int64_t)1 << 30) || total_obs > ((int64_t)1 << 30)) return "the map holds more than 2^30 slots or observations";
    return nullptr;
}

}  // namespace sivo
