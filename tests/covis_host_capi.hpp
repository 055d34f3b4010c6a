// covis_host_capi.hpp — sivo_covis_count, sivo_keyframe_culling and sivo_mappoint_culling of include/sivo_hip.h over the HOST build of the
// kernels' per-slot bodies (sivo_amd/csrc/covis_math.hpp), with the argument checks of the library (the same functions of that header) and
// the results stored as covis.hip stores them (the counts of a keyframe skipped as id 0 left as the caller had them).  Sequential loops in
// place of the launches: no library, no device, so the programs that include it (tests/covis_prog.cpp, tests/covis_adapter_prog.cpp) can
// run under the sanitizers.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "covis_math.hpp"

namespace covis_host {
inline std::string &error() { static std::string e; return e; }
inline int fail(const char *where, const char *what) { error() = std::string(where) + ": " + what; return SIVO_ERR_INVALID_ARGUMENT; }
inline long &calls() { static long n = 0; return n; }        // how many entry-point calls were made (the adapter's "one launch" claims)
}  // namespace covis_host

extern "C" {

const char *sivo_last_error(void) { return covis_host::error().c_str(); }

int sivo_covis_count(const SivoObsTable *t, int n_sets, const int64_t *set_off, const int32_t *set_point, const int32_t *set_self,
                            int32_t *counts) {
    ++covis_host::calls();
    if (const char *e = sivo::cv_check_count(t, n_sets, set_off, set_point, set_self, counts)) return covis_host::fail("sivo_covis_count", e);
    if (n_sets == 0 || t->n_kf == 0) return SIVO_OK;
    std::memset(counts, 0, sizeof(int32_t) * (size_t)n_sets * (size_t)t->n_kf);
    for (int s = 0; s < n_sets; ++s) {
        int32_t *row = counts + (size_t)s * (size_t)t->n_kf;
        for (int64_t i = set_off[s]; i < set_off[s + 1]; ++i) sivo::cv_count_slot(*t, set_point[i], set_self[s], [&](int32_t k) { ++row[k]; });
    }
    return SIVO_OK;
}

int sivo_keyframe_culling(const SivoObsTable *t, int n_local, const int32_t *local_kf, const uint8_t *is_id0, const uint8_t *erasable,
                                 const float *th_depth, const int64_t *slot_off, const int32_t *slot_point, const uint8_t *slot_level,
                                 const float *slot_depth, int monocular, int32_t *n_mps, int32_t *n_redundant, uint8_t *decision,
                                 uint8_t *bad_after) {
    ++covis_host::calls();
    if (const char *e = sivo::cv_check_kfcull(t, n_local, local_kf, is_id0, erasable, th_depth, slot_off, slot_point, slot_level, slot_depth, n_mps,
                                              n_redundant, decision, bad_after))
        return covis_host::fail("sivo_keyframe_culling", e);
    if (t->n_points) std::memcpy(bad_after, t->point_bad, (size_t)t->n_points);
    std::vector<uint8_t> removed((size_t)t->n_kf + 1, 0);
    for (int j = 0; j < n_local; ++j) {
        if (is_id0[j]) { decision[j] = SIVO_KFCULL_ID0; continue; }
        const int32_t kf = local_kf[j];
        int32_t mps = 0, red = 0;
        for (int64_t i = slot_off[j]; i < slot_off[j + 1]; ++i) {
            const sivo::CvSlot r = sivo::cv_kf_slot(*t, bad_after, removed.data(), kf, slot_point[i], slot_level[i], slot_depth[i], th_depth[j], monocular != 0);
            mps += r.counted; red += r.redundant;
        }
        n_mps[j] = mps; n_redundant[j] = red;
        decision[j] = sivo::cv_kf_decision(red, mps, erasable[j]);
        if (decision[j] != SIVO_KFCULL_CULLED) continue;
        for (int64_t i = slot_off[j]; i < slot_off[j + 1]; ++i)
            if (sivo::cv_kf_slot(*t, bad_after, removed.data(), kf, slot_point[i], slot_level[i], slot_depth[i], th_depth[j], monocular != 0).goes_bad)
                bad_after[slot_point[i]] = 1;
        removed[(size_t)kf] = 1;
    }
    return SIVO_OK;
}

int sivo_mappoint_culling(int n, const int32_t *found, const int32_t *visible, const int64_t *first_kf_id, const int32_t *n_obs,
                                 const uint8_t *bad, int64_t current_kf_id, int monocular, uint8_t *status) {
    ++covis_host::calls();
    if (const char *e = sivo::cv_check_mpcull(n, found, visible, first_kf_id, n_obs, bad, status)) return covis_host::fail("sivo_mappoint_culling", e);
    for (int i = 0; i < n; ++i) status[i] = sivo::cv_mappoint_status(found[i], visible[i], first_kf_id[i], n_obs[i], bad[i], current_kf_id, monocular != 0);
    return SIVO_OK;
}

}  // extern "C"
