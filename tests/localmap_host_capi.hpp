// localmap_host_capi.hpp — the sivo_localmap_* entry points of include/sivo_hip.h over the HOST build of the kernels' per-item bodies
// (sivo_amd/csrc/localmap_math.hpp), with the argument checks of the library (the same functions of that header) and the results stored as
// localmap.hip stores them (nothing on SIVO_ERR_CAPACITY, local_kf untouched where nobody voted, nothing past the counts).  Sequential
// loops in place of the launches and a plain struct for the handle: no library, no device, so the programs that include it
// (tests/localmap_prog.cpp, tests/localmap_adapter_prog.cpp) can run under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "localmap_math.hpp"

namespace localmap_host {
inline std::string &error() { static std::string e; return e; }
inline int fail(int code, const char *where, const std::string &what) { error() = std::string(where) + ": " + what; return code; }
inline long &calls() { static long n = 0; return n; }        // how many sivo_localmap_update calls were made (the adapter's "one call")
}  // namespace localmap_host

struct sivo_localmap {
    std::vector<int64_t> obs_off, slot_off, covis_off, child_off;
    std::vector<int32_t> obs_kf, slot_point, covis_kf, child_kf, parent, kf_order;
    std::vector<uint8_t> point_bad, kf_bad;
    SivoLocalMapTables t;

    void load(const SivoLocalMapTables &s) {
        const size_t K = (size_t)s.n_kf, P = (size_t)s.n_points;
        auto off = [](const int64_t *p, size_t n) { return n ? std::vector<int64_t>(p, p + n + 1) : std::vector<int64_t>(1, 0); };
        auto i32 = [](const int32_t *p, size_t n) { return n ? std::vector<int32_t>(p, p + n) : std::vector<int32_t>(); };
        auto u8 = [](const uint8_t *p, size_t n) { return n ? std::vector<uint8_t>(p, p + n) : std::vector<uint8_t>(); };
        obs_off = off(s.obs_off, P); obs_kf = i32(s.obs_kf, (size_t)obs_off.back()); point_bad = u8(s.point_bad, P); kf_bad = u8(s.kf_bad, K);
        slot_off = off(s.slot_off, K); slot_point = i32(s.slot_point, (size_t)slot_off.back());
        covis_off = off(s.covis_off, K); covis_kf = i32(s.covis_kf, (size_t)covis_off.back());
        child_off = off(s.child_off, K); child_kf = i32(s.child_kf, (size_t)child_off.back());
        parent = i32(s.parent, K);
        kf_order.resize(K);
        for (size_t k = 0; k < K; ++k) kf_order[k] = s.kf_order ? s.kf_order[k] : (int32_t)k;
        t.n_kf = s.n_kf; t.n_points = s.n_points;
        t.obs_off = obs_off.data(); t.obs_kf = obs_kf.data(); t.point_bad = point_bad.data(); t.kf_bad = kf_bad.data();
        t.slot_off = slot_off.data(); t.slot_point = slot_point.data(); t.covis_off = covis_off.data(); t.covis_kf = covis_kf.data();
        t.child_off = child_off.data(); t.child_kf = child_kf.data(); t.parent = parent.data(); t.kf_order = kf_order.data();
    }
};

extern "C" {

const char *sivo_last_error(void) { return localmap_host::error().c_str(); }

int sivo_localmap_create(const SivoLocalMapTables *t, sivo_localmap_t *map) {
    if (!map) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_create", "null handle pointer");
    *map = nullptr;
    if (const char *e = sivo::lm_check_tables(t)) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_create", e);
    *map = new sivo_localmap;
    (*map)->load(*t);
    return SIVO_OK;
}

int sivo_localmap_replace(sivo_localmap_t m, const SivoLocalMapTables *t) {
    if (!m) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_replace", "null handle");
    if (const char *e = sivo::lm_check_tables(t)) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_replace", e);
    m->load(*t);
    return SIVO_OK;
}

int sivo_localmap_destroy(sivo_localmap_t m) {
    delete m;
    return SIVO_OK;
}

int sivo_localmap_set_bad(sivo_localmap_t m, int n_points, const int32_t *point_idx, const uint8_t *point_val, int n_kf, const int32_t *kf_idx,
                          const uint8_t *kf_val) {
    if (!m) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_set_bad", "null handle");
    if (const char *e = sivo::lm_check_set_bad(m->t.n_kf, m->t.n_points, n_points, point_idx, point_val, n_kf, kf_idx, kf_val))
        return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_set_bad", e);
    for (int i = 0; i < n_points; ++i) m->point_bad[(size_t)point_idx[i]] = point_val[i] ? 1 : 0;
    for (int i = 0; i < n_kf; ++i) m->kf_bad[(size_t)kf_idx[i]] = kf_val[i] ? 1 : 0;
    return SIVO_OK;
}

int sivo_localmap_update(sivo_localmap_t m, int n_slots, const int32_t *frame_point, int n_kf_premarked, const int32_t *kf_premarked,
                         int n_point_premarked, const int32_t *point_premarked, int n_prev, const int32_t *prev_local_kf, int32_t *voted,
                         uint8_t *slot_cleared, int kf_capacity, int32_t *local_kf, int32_t *n_local_kf, int32_t *ref_kf, int point_capacity,
                         int32_t *local_point, int32_t *n_local_points, int32_t *counts) {
    using namespace sivo;
    ++localmap_host::calls();
    if (!m) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_update", "null handle");
    const SivoLocalMapTables &t = m->t;
    int64_t g_prev = 0;
    if (const char *e = lm_check_update(t.n_kf, t.n_points, t.slot_off, n_slots, frame_point, n_kf_premarked, kf_premarked, n_point_premarked,
                                        point_premarked, n_prev, prev_local_kf, voted, slot_cleared, kf_capacity, local_kf, n_local_kf, ref_kf,
                                        point_capacity, local_point, n_local_points, &g_prev))
        return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_update", e);
    const size_t K = (size_t)t.n_kf, P = (size_t)t.n_points;
    // the vote kernel
    const SivoObsTable o = lm_obs_table(t);
    std::vector<int32_t> cnt(K + 1, 0);
    std::vector<uint8_t> cleared((size_t)n_slots + 1, 0);
    for (int i = 0; i < n_slots; ++i) {
        cleared[(size_t)i] = lm_slot_cleared(t, frame_point[i]);
        cv_count_slot(o, frame_point[i], -1, [&](int32_t k) { ++cnt[(size_t)k]; });
    }
    // the select kernel
    std::vector<uint32_t> marks((K + 31) / 32 + 1, 0), first(P + 1, LM_FIRST_NONE);
    for (int i = 0; i < n_kf_premarked; ++i) marks[(size_t)(kf_premarked[i] >> 5)] |= lm_mark_bit(kf_premarked[i]);
    for (int i = 0; i < n_point_premarked; ++i) first[(size_t)point_premarked[i]] = LM_FIRST_PREMARKED;
    bool any = false;
    for (size_t k = 0; k < K; ++k) any = any || cnt[k] > 0;
    std::vector<int32_t> local;
    uint64_t best = 0;
    auto push = [&](int32_t k) { local.push_back(k); marks[(size_t)(k >> 5)] |= lm_mark_bit(k); };
    if (any) {
        for (int32_t i = 0; i < t.n_kf; ++i) {                          // stage 1
            const int32_t k = t.kf_order[i];
            if (!lm_stage1_takes(t, cnt.data(), k)) continue;
            push(k);
            best = std::max(best, lm_max_key(cnt[(size_t)k], i));
        }
        const size_t n1 = local.size();
        for (size_t j = 0; j < n1; ++j) {                               // stage 2
            if (local.size() > (size_t)LM_MAX_LOCAL) break;
            const int32_t k = local[j];
            const int64_t c0 = t.covis_off[k], cn = std::min<int64_t>(t.covis_off[k + 1] - c0, LM_BEST_COVIS);
            for (int64_t c = c0; c < c0 + cn; ++c)
                if (lm_neighbour_ok(t, marks.data(), t.covis_kf[c])) { push(t.covis_kf[c]); break; }
            for (int64_t c = t.child_off[k]; c < t.child_off[k + 1]; ++c)
                if (lm_neighbour_ok(t, marks.data(), t.child_kf[c])) { push(t.child_kf[c]); break; }
            const int32_t par = t.parent[k];
            if (par >= 0 && !lm_marked(marks.data(), par)) { push(par); break; }
        }
    }
    const int32_t *list = any ? local.data() : prev_local_kf;
    const int32_t n_list = any ? (int32_t)local.size() : n_prev;
    std::vector<int32_t> list_off((size_t)n_list + 1, 0);
    for (int32_t i = 0; i < n_list; ++i) list_off[(size_t)i + 1] = list_off[(size_t)i] + (int32_t)(t.slot_off[list[i] + 1] - t.slot_off[list[i]]);
    const int32_t G = list_off[(size_t)n_list];
    // the point kernels: pass 1, then pass 2
    for (int32_t g = 0; g < G; ++g) {
        const int32_t p = lm_slot_point(t, list, list_off.data(), n_list, g);
        if (p >= 0) first[(size_t)p] = std::min(first[(size_t)p], (uint32_t)g + 1u);
    }
    std::vector<int32_t> pts;
    for (int32_t g = 0; g < G; ++g) {
        const int32_t p = lm_slot_point(t, list, list_off.data(), n_list, g);
        if (lm_point_survives(t, first.data(), p, g)) pts.push_back(p);
    }
    char text[96];
    if (any && (int64_t)local.size() > kf_capacity) {
        std::snprintf(text, sizeof text, "%d local keyframes, capacity %d", (int)local.size(), kf_capacity);
        return localmap_host::fail(SIVO_ERR_CAPACITY, "sivo_localmap_update", text);
    }
    if ((int64_t)pts.size() > point_capacity) {
        std::snprintf(text, sizeof text, "%d local map points, capacity %d", (int)pts.size(), point_capacity);
        return localmap_host::fail(SIVO_ERR_CAPACITY, "sivo_localmap_update", text);
    }
    *voted = any ? 1 : 0;
    if (n_slots) std::memcpy(slot_cleared, cleared.data(), (size_t)n_slots);
    if (any) {
        *n_local_kf = (int32_t)local.size();
        if (!local.empty()) std::memcpy(local_kf, local.data(), 4 * local.size());
    }
    *ref_kf = best ? t.kf_order[lm_key_pos(best)] : -1;
    *n_local_points = (int32_t)pts.size();
    if (!pts.empty()) std::memcpy(local_point, pts.data(), 4 * pts.size());
    if (counts && K) std::memcpy(counts, cnt.data(), 4 * K);
    return SIVO_OK;
}

}  // extern "C"
