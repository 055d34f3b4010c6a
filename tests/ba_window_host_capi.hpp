// ba_window_host_capi.hpp — sivo_localmap_ba_window of include/sivo_hip.h over the HOST build of the kernels' per-item bodies
// (sivo_amd/csrc/ba_window_math.hpp and localmap_math.hpp), with the argument check of the library (the same function of that header) and
// the results stored as ba_window.hip stores them (counts on success and on SIVO_ERR_CAPACITY, where nothing else is written; nothing past
// the counts).  Sequential loops in place of the launches, on the handle of tests/localmap_host_capi.hpp: no library, no device, so the
// programs that include it (tests/ba_window_prog.cpp, tests/ba_window_adapter_prog.cpp) can run under the sanitizers.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "localmap_host_capi.hpp"

#include "ba_window_math.hpp"

namespace ba_window_host {
inline long &calls() { static long n = 0; return n; }        // how many sivo_localmap_ba_window calls were made (the adapter's "one call")
inline double &seconds() { static double s = 0; return s; }  // the time spent in them (tools/ba_window_probe.py takes it off the gather's)
struct Clock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~Clock() { seconds() += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
}  // namespace ba_window_host

extern "C" int sivo_localmap_ba_window(sivo_localmap_t m, int n_cand, const int32_t *cand_kf, int n_kf_local_pre, const int32_t *kf_local_pre,
                                       int n_kf_fixed_pre, const int32_t *kf_fixed_pre, int n_point_pre, const int32_t *point_pre, int kf_capacity,
                                       int32_t *local_kf, int32_t *fixed_kf, int point_capacity, int32_t *local_point, int64_t *edge_off,
                                       int64_t edge_capacity, int32_t *edge_pose, int32_t *edge_slot, int64_t counts[4]) {
    using namespace sivo;
    const char *const where = "sivo_localmap_ba_window";
    ++ba_window_host::calls();
    const ba_window_host::Clock clock;
    if (!m) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, where, "null handle");
    const SivoLocalMapTables &t = m->t;
    const size_t K = (size_t)t.n_kf, P = (size_t)t.n_points;
    if (const char *e = bw_check_window(t.n_kf, t.n_points, m->slot_off.back(), m->obs_off.back(), n_cand, cand_kf, n_kf_local_pre, kf_local_pre,
                                        n_kf_fixed_pre, kf_fixed_pre, n_point_pre, point_pre, kf_capacity, local_kf, fixed_kf, point_capacity,
                                        local_point, edge_off, edge_capacity, edge_pose, edge_slot, counts))
        return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, where, e);
    // the select kernel
    std::vector<uint32_t> kf_first(K + 1, BW_FIRST_NONE), first(P + 1, LM_FIRST_NONE);
    std::vector<int32_t> pose_of(K + 1, -1), local;
    for (int i = 0; i < n_cand; ++i) kf_first[(size_t)cand_kf[i]] = BW_FIRST_MARKED;
    for (int i = 0; i < n_kf_local_pre; ++i) kf_first[(size_t)kf_local_pre[i]] = BW_FIRST_MARKED;
    for (int i = 0; i < n_kf_fixed_pre; ++i) kf_first[(size_t)kf_fixed_pre[i]] = BW_FIRST_MARKED;
    for (int i = 0; i < n_point_pre; ++i) first[(size_t)point_pre[i]] = LM_FIRST_PREMARKED;
    for (int32_t i = 0; i < n_cand; ++i)
        if (bw_cand_listed(t, cand_kf, i)) {
            pose_of[(size_t)cand_kf[i]] = (int32_t)local.size();
            local.push_back(cand_kf[i]);
        }
    const int32_t n_local = (int32_t)local.size();
    std::vector<int32_t> list_off((size_t)n_local + 1, 0);
    for (int32_t i = 0; i < n_local; ++i) list_off[(size_t)i + 1] = list_off[(size_t)i] + (int32_t)(t.slot_off[local[(size_t)i] + 1] - t.slot_off[local[(size_t)i]]);
    const int32_t G = list_off[(size_t)n_local];
    // the point kernels: pass 1, then pass 2
    for (int32_t g = 0; g < G; ++g) {
        const int32_t p = lm_slot_point(t, local.data(), list_off.data(), n_local, g);
        if (p >= 0) first[(size_t)p] = std::min(first[(size_t)p], (uint32_t)g + 1u);
    }
    std::vector<int32_t> pts;
    for (int32_t g = 0; g < G; ++g) {
        const int32_t p = lm_slot_point(t, local.data(), list_off.data(), n_local, g);
        if (lm_point_survives(t, first.data(), p, g)) pts.push_back(p);
    }
    pts.push_back(0);                                                   // (never read: data() of an empty vector may be null)
    const int32_t n_pts = (int32_t)pts.size() - 1;
    // the row offsets, then the fixed kernels: pass 1, then pass 2
    std::vector<int32_t> row_off((size_t)n_pts + 1, 0);
    for (int32_t i = 0; i < n_pts; ++i) row_off[(size_t)i + 1] = row_off[(size_t)i] + bw_row_len(t, pts.data(), i);
    const int32_t H = row_off[(size_t)n_pts];
    for (int32_t h = 0; h < H; ++h) {
        const BwObs o = bw_obs(t, pts.data(), row_off.data(), n_pts, h);
        kf_first[(size_t)o.k] = std::min(kf_first[(size_t)o.k], (uint32_t)h + 1u);
    }
    std::vector<int32_t> fixed;
    for (int32_t h = 0; h < H; ++h) {
        const BwObs o = bw_obs(t, pts.data(), row_off.data(), n_pts, h);
        if (!bw_fixed_survives(t, kf_first.data(), o.k, h)) continue;
        pose_of[(size_t)o.k] = n_local + (int32_t)fixed.size();
        fixed.push_back(o.k);
    }
    // the edge offsets, then the edge kernel
    std::vector<int64_t> eoff((size_t)n_pts + 1, 0);
    for (int32_t i = 0; i < n_pts; ++i) eoff[(size_t)i + 1] = eoff[(size_t)i] + bw_kept_before(t, pose_of.data(), pts[(size_t)i], bw_row_len(t, pts.data(), i));
    const int64_t n_edges = eoff[(size_t)n_pts];
    std::vector<int32_t> epose((size_t)n_edges + 1, 0), eslot((size_t)n_edges + 1, 0);
    for (int32_t h = 0; h < H; ++h) {
        const BwObs o = bw_obs(t, pts.data(), row_off.data(), n_pts, h);
        if (!bw_edge_kept(t, pose_of.data(), o.k)) continue;
        const int64_t e = eoff[(size_t)o.i] + bw_kept_before(t, pose_of.data(), o.p, o.r);
        const int32_t len = (int32_t)(t.slot_off[o.k + 1] - t.slot_off[o.k]);
        int32_t hits = 0, lowest = -1;
        for (int32_t s = 0; s < len; ++s)
            if (bw_slot_hit(t, o.k, s, o.p)) {
                if (!hits) lowest = s;
                ++hits;
            }
        epose[(size_t)e] = pose_of[(size_t)o.k];
        eslot[(size_t)e] = bw_slot_code(hits, lowest);
    }
    counts[0] = n_local; counts[1] = n_pts; counts[2] = (int64_t)fixed.size(); counts[3] = n_edges;
    char text[128];
    if (n_local > kf_capacity || (int64_t)fixed.size() > kf_capacity) {
        std::snprintf(text, sizeof text, "%d local and %d fixed keyframes, capacity %d", n_local, (int)fixed.size(), kf_capacity);
        return localmap_host::fail(SIVO_ERR_CAPACITY, where, text);
    }
    if (n_pts > point_capacity) {
        std::snprintf(text, sizeof text, "%d local map points, capacity %d", n_pts, point_capacity);
        return localmap_host::fail(SIVO_ERR_CAPACITY, where, text);
    }
    if (n_edges > edge_capacity) {
        std::snprintf(text, sizeof text, "%d edges, capacity %lld", (int)n_edges, (long long)edge_capacity);
        return localmap_host::fail(SIVO_ERR_CAPACITY, where, text);
    }
    if (n_local) std::memcpy(local_kf, local.data(), 4 * (size_t)n_local);
    if (!fixed.empty()) std::memcpy(fixed_kf, fixed.data(), 4 * fixed.size());
    if (n_pts) std::memcpy(local_point, pts.data(), 4 * (size_t)n_pts);
    std::memcpy(edge_off, eoff.data(), 8 * ((size_t)n_pts + 1));
    if (n_edges) {
        std::memcpy(edge_pose, epose.data(), 4 * (size_t)n_edges);
        std::memcpy(edge_slot, eslot.data(), 4 * (size_t)n_edges);
    }
    return SIVO_OK;
}
