// localmap_delta_math.hpp — the per-item bodies of sivo_localmap_apply: how a resident set of CSR tables (localmap_math.hpp) takes a delta
// of replaced and appended rows, and the argument check of the delta; shared by the kernels (localmap.hip) and, compiled by g++, by the
// host programs of the tests (tests/localmap_delta_host_capi.hpp).  Integers throughout.
//
// Each of the four CSR tables (obs over the points; slots, covisibles and children over the keyframes) goes through four passes:
//   mark     delta row j stamps j + 1 into src[idx[j]]; src is zeroed and as long as the NEW row count, one src[] serves the three keyframe
//            tables.  The indices are strictly increasing, so no entry is stamped twice.
//   length   new row r is as long as delta row src[r] - 1 where src[r] is set, else as long as it was.
//   scan     the exclusive prefix of the lengths is the new offset array, its last entry the table's new total.
//   gather   new row r is copied entry by entry from the delta's pool or from the old pool.
// point_bad, kf_bad, parent and kf_order are copied and the delta's rows scattered over the copy.
#pragma once
#include <stdint.h>

#include <vector>

#include "localmap_math.hpp"

namespace sivo {

enum { LMD_OBS = 0, LMD_SLOT, LMD_COVIS, LMD_CHILD, LMD_TABLES };

// one CSR table under a delta: the old table, the delta's rows and the table that is built
struct LmdCsr {
    int32_t n_old, n_new;           // rows before and after
    const int64_t *old_off;         // n_old + 1; not read where n_old == 0
    const int32_t *old_val;
    const int64_t *d_off;           // the delta's rows (n_rows + 1) and their pool
    const int32_t *d_val;
    const int32_t *src;             // n_new: 0, or 1 + the delta row that replaces the row
    int64_t *new_off;               // n_new + 1
    int32_t *new_val;
};

// mark: delta row j replaces (or is) row idx[j]
SIVO_HD void lmd_mark(int32_t *src, const int32_t *idx, int32_t j) { src[idx[j]] = j + 1; }

// length of new row r; a row at or behind n_old is always a delta row (the check refuses a delta that does not list it)
SIVO_HD int32_t lmd_row_len(const LmdCsr &c, int32_t r) {
    const int32_t s = c.src[r];
    if (s) return (int32_t)(c.d_off[s] - c.d_off[s - 1]);
    return (int32_t)(c.old_off[r + 1] - c.old_off[r]);
}

// gather: where entry 0 of new row r comes from
SIVO_HD const int32_t *lmd_row_source(const LmdCsr &c, int32_t r) {
    const int32_t s = c.src[r];
    return s ? c.d_val + c.d_off[s - 1] : c.old_val + c.old_off[r];
}

// ---- the argument check, host only: the text of what is wrong, or nullptr -------------------------------------------------------------
inline const char *lmd_check_rows(const int32_t *idx, int32_t n_rows, int32_t n_old, int32_t n_new, const char *null_text, const char *order_text,
                                  const char *range_text, const char *unlisted_text) {
    if (n_rows && !idx) return null_text;
    for (int32_t j = 0; j < n_rows; ++j) {
        if (idx[j] < 0 || idx[j] >= n_new) return range_text;
        if (j && idx[j] <= idx[j - 1]) return order_text;
    }
    const int32_t added = n_new - n_old;                // strictly increasing below n_new: the new rows are the tail of the list, or one is missing
    if (added > n_rows || (added && idx[n_rows - added] != n_old)) return unlisted_text;
    return nullptr;
}

// n_kf_map, n_points_map and total[LMD_TABLES] are the handle's; header_size = sizeof(SivoLocalMapDelta) of the build that checks
inline const char *lmd_check_delta(int32_t n_kf_map, int32_t n_points_map, const int64_t *total, const SivoLocalMapDelta *d, size_t header_size) {
    if (!d) return "null delta";
    if ((size_t)d->size != header_size) return "size is not sizeof(SivoLocalMapDelta)";
    if (d->n_kf < 0 || d->n_points < 0 || d->n_point_rows < 0 || d->n_kf_rows < 0) return "negative count";
    if (d->n_kf < n_kf_map) return "n_kf is smaller than the handle's";
    if (d->n_points < n_points_map) return "n_points is smaller than the handle's";
    if (d->n_kf > (1 << 24) || d->n_points > (1 << 24)) return "more than 2^24 keyframes or points";
    const int32_t K = d->n_kf, P = d->n_points, np = d->n_point_rows, nk = d->n_kf_rows;
    if (const char *e = lmd_check_rows(d->point_idx, np, n_points_map, P, "null point_idx", "point_idx is not strictly increasing",
                                       "point_idx outside 0 .. n_points - 1", "point_idx does not list every appended point")) return e;
    if (const char *e = lmd_check_rows(d->kf_idx, nk, n_kf_map, K, "null kf_idx", "kf_idx is not strictly increasing", "kf_idx outside 0 .. n_kf - 1",
                                       "kf_idx does not list every appended keyframe")) return e;
    if (np) {
        if (const char *e = cv_check_csr(d->point_obs_off, np, "null point_obs_off", "point_obs_off does not start at 0", "point_obs_off decreases")) return e;
        if (const char *e = cv_check_index(d->point_obs_kf, d->point_obs_off[np], 0, K, "null point_obs_kf", "point_obs_kf outside 0 .. n_kf - 1")) return e;
        if (!d->point_bad) return "null point_bad";
        if (total[LMD_OBS] + d->point_obs_off[np] > ((int64_t)1 << 28)) return "point_obs_kf: more than 2^28 entries with the handle's";
    }
    if (nk) {
        if (!d->kf_bad) return "null kf_bad";
        if (const char *e = cv_check_index(d->kf_parent, nk, -1, K, "null kf_parent", "kf_parent outside -1 .. n_kf - 1")) return e;
        if (const char *e = cv_check_csr(d->kf_slot_off, nk, "null kf_slot_off", "kf_slot_off does not start at 0", "kf_slot_off decreases")) return e;
        if (const char *e = cv_check_index(d->kf_slot_point, d->kf_slot_off[nk], -1, P, "null kf_slot_point", "kf_slot_point outside -1 .. n_points - 1")) return e;
        if (const char *e = cv_check_csr(d->kf_covis_off, nk, "null kf_covis_off", "kf_covis_off does not start at 0", "kf_covis_off decreases")) return e;
        if (const char *e = cv_check_index(d->kf_covis_kf, d->kf_covis_off[nk], 0, K, "null kf_covis_kf", "kf_covis_kf outside 0 .. n_kf - 1")) return e;
        if (const char *e = cv_check_csr(d->kf_child_off, nk, "null kf_child_off", "kf_child_off does not start at 0", "kf_child_off decreases")) return e;
        if (const char *e = cv_check_index(d->kf_child_kf, d->kf_child_off[nk], 0, K, "null kf_child_kf", "kf_child_kf outside 0 .. n_kf - 1")) return e;
        if (total[LMD_SLOT] + d->kf_slot_off[nk] > ((int64_t)1 << 28)) return "kf_slot_point: more than 2^28 entries with the handle's";
        if (total[LMD_COVIS] + d->kf_covis_off[nk] > ((int64_t)1 << 28)) return "kf_covis_kf: more than 2^28 entries with the handle's";
        if (total[LMD_CHILD] + d->kf_child_off[nk] > ((int64_t)1 << 28)) return "kf_child_kf: more than 2^28 entries with the handle's";
    }
    if (d->kf_order) {
        std::vector<uint8_t> seen((size_t)K, 0);
        for (int32_t i = 0; i < K; ++i) {
            const int32_t k = d->kf_order[i];
            if (k < 0 || k >= K || seen[(size_t)k]) return "kf_order is not a permutation of 0 .. n_kf - 1";
            seen[(size_t)k] = 1;
        }
    }
    return nullptr;
}

// no rows, the handle's sizes, no order: nothing to do
inline bool lmd_is_empty(int32_t n_kf_map, int32_t n_points_map, const SivoLocalMapDelta &d) {
    return d.n_point_rows == 0 && d.n_kf_rows == 0 && d.n_kf == n_kf_map && d.n_points == n_points_map && !d.kf_order;
}

// sivo_localmap_export: the caller's arrays for a handle of these sizes
inline const char *lmd_check_export(int32_t n_kf_map, int32_t n_points_map, const int64_t *total, const SivoLocalMapTables *out) {
    if (!out) return "null tables";
    if (out->n_kf != n_kf_map) return "n_kf is not the handle's";
    if (out->n_points != n_points_map) return "n_points is not the handle's";
    if (n_points_map && (!out->obs_off || !out->point_bad)) return "null obs_off or point_bad";
    if (total[LMD_OBS] && !out->obs_kf) return "null obs_kf";
    if (n_kf_map && (!out->kf_bad || !out->slot_off || !out->covis_off || !out->child_off || !out->parent || !out->kf_order)) return "null keyframe array";
    if (total[LMD_SLOT] && !out->slot_point) return "null slot_point";
    if (total[LMD_COVIS] && !out->covis_kf) return "null covis_kf";
    if (total[LMD_CHILD] && !out->child_kf) return "null child_kf";
    return nullptr;
}

// the delta's part of table w
inline void lmd_delta_table(const SivoLocalMapDelta &d, int w, const int64_t *&off, const int32_t *&val) {
    switch (w) {
    case LMD_OBS: off = d.point_obs_off; val = d.point_obs_kf; break;
    case LMD_SLOT: off = d.kf_slot_off; val = d.kf_slot_point; break;
    case LMD_COVIS: off = d.kf_covis_off; val = d.kf_covis_kf; break;
    default: off = d.kf_child_off; val = d.kf_child_kf; break;
    }
}

// What the host keeps of the slot table (the update's grid bound and argument check read it): the new slot_off from the old one and the
// delta's rows, in O(keyframes).
inline std::vector<int64_t> lmd_host_slot_off(const std::vector<int64_t> &old_off, int32_t n_kf_old, const SivoLocalMapDelta &d) {
    std::vector<int64_t> len((size_t)d.n_kf, 0), off((size_t)d.n_kf + 1, 0);
    for (int32_t k = 0; k < n_kf_old; ++k) len[(size_t)k] = old_off[(size_t)k + 1] - old_off[(size_t)k];
    for (int32_t j = 0; j < d.n_kf_rows; ++j) len[(size_t)d.kf_idx[j]] = d.kf_slot_off[j + 1] - d.kf_slot_off[j];
    for (int32_t k = 0; k < d.n_kf; ++k) off[(size_t)k + 1] = off[(size_t)k] + len[(size_t)k];
    return off;
}

}  // namespace sivo
