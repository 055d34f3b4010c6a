// localmap_delta_host_capi.hpp — sivo_localmap_apply, _sizes and _export of include/sivo_hip.h over the HOST build of the kernels' per-item
// bodies (sivo_amd/csrc/localmap_delta_math.hpp), beside the entry points of localmap_host_capi.hpp, which it includes unchanged: the
// library's check of the delta (the same function of that header), then the four passes of localmap.hip in sequence over each table —
// mark, length per block of 256, the scan with the sum of the blocks before it, the gather — in sequential loops in place of the
// launches.  No library, no device: the programs that include it run under the sanitizers.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "localmap_delta_math.hpp"
#include "localmap_host_capi.hpp"

namespace localmap_host {
inline long &applies() { static long n = 0; return n; }      // how many sivo_localmap_apply calls were made (the adapter's "one call")
constexpr int LP_THREADS = 256;                              // the block of the scan in localmap.hip
inline void totals(const sivo_localmap &m, int64_t t[sivo::LMD_TABLES]) {
    t[sivo::LMD_OBS] = m.obs_off.back(); t[sivo::LMD_SLOT] = m.slot_off.back(); t[sivo::LMD_COVIS] = m.covis_off.back();
    t[sivo::LMD_CHILD] = m.child_off.back();
}
}  // namespace localmap_host

extern "C" {

int sivo_localmap_apply(sivo_localmap_t m, const SivoLocalMapDelta *dl) {
    using namespace sivo;
    ++localmap_host::applies();
    if (!m) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_apply", "null handle");
    int64_t total[LMD_TABLES];
    localmap_host::totals(*m, total);
    if (const char *e = lmd_check_delta(m->t.n_kf, m->t.n_points, total, dl, sizeof(SivoLocalMapDelta)))
        return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_apply", e);
    if (lmd_is_empty(m->t.n_kf, m->t.n_points, *dl)) return SIVO_OK;
    const SivoLocalMapDelta &d = *dl;
    const int32_t K0 = m->t.n_kf, P0 = m->t.n_points, K1 = d.n_kf, P1 = d.n_points;
    // mark
    std::vector<int32_t> src_p((size_t)P1 + 1, 0), src_k((size_t)K1 + 1, 0);
    for (int32_t j = 0; j < d.n_point_rows; ++j) lmd_mark(src_p.data(), d.point_idx, j);
    for (int32_t j = 0; j < d.n_kf_rows; ++j) lmd_mark(src_k.data(), d.kf_idx, j);
    const std::vector<int64_t> *old_off[LMD_TABLES] = {&m->obs_off, &m->slot_off, &m->covis_off, &m->child_off};
    const std::vector<int32_t> *old_val[LMD_TABLES] = {&m->obs_kf, &m->slot_point, &m->covis_kf, &m->child_kf};
    std::vector<int64_t> new_off[LMD_TABLES];
    std::vector<int32_t> new_val[LMD_TABLES];
    for (int w = 0; w < LMD_TABLES; ++w) {
        LmdCsr c;
        c.n_old = w == LMD_OBS ? P0 : K0; c.n_new = w == LMD_OBS ? P1 : K1;
        c.old_off = old_off[w]->data(); c.old_val = old_val[w]->data();
        lmd_delta_table(d, w, c.d_off, c.d_val);
        c.src = w == LMD_OBS ? src_p.data() : src_k.data();
        const int T = localmap_host::LP_THREADS, nb = (c.n_new + T - 1) / T;
        // length: the sum of every block of rows
        std::vector<int32_t> block_sum((size_t)nb + 1, 0);
        for (int32_t r = 0; r < c.n_new; ++r) block_sum[(size_t)(r / T)] += lmd_row_len(c, r);
        // scan: inside the block, behind the sum of the blocks before it
        new_off[w].assign((size_t)c.n_new + 1, 0);
        c.new_off = new_off[w].data();
        int64_t total_w = 0;
        for (int blk = 0; blk < nb; ++blk) {
            int64_t base = 0;
            for (int b = 0; b < blk; ++b) base += block_sum[(size_t)b];
            int32_t excl = 0;
            for (int32_t r = blk * T; r < std::min(c.n_new, (blk + 1) * T); ++r) {
                c.new_off[r] = base + excl;
                excl += lmd_row_len(c, r);
                if (r == c.n_new - 1) total_w = c.new_off[c.n_new] = base + excl;
            }
        }
        // gather: sized, as in the library, from the bound old total + delta total
        const size_t rows = (size_t)(w == LMD_OBS ? d.n_point_rows : d.n_kf_rows);
        new_val[w].assign((size_t)total[w] + (rows ? (size_t)c.d_off[rows] : 0), 0);
        c.new_val = new_val[w].data();
        for (int32_t r = 0; r < c.n_new; ++r) {
            const int64_t at = c.new_off[r];
            const int32_t len = (int32_t)(c.new_off[r + 1] - at);
            const int32_t *from = lmd_row_source(c, r);
            for (int32_t e = 0; e < len; ++e) c.new_val[at + e] = from[e];
        }
        new_val[w].resize((size_t)total_w);                             // the exact total is what is kept
    }
    // the flags, the parents and the order: copies, then the delta's rows over them
    std::vector<uint8_t> point_bad(m->point_bad), kf_bad(m->kf_bad);
    std::vector<int32_t> parent(m->parent), kf_order(m->kf_order);
    point_bad.resize((size_t)P1, 0); kf_bad.resize((size_t)K1, 0); parent.resize((size_t)K1, -1); kf_order.resize((size_t)K1, -1);
    for (int32_t j = 0; j < d.n_point_rows; ++j) point_bad[(size_t)d.point_idx[j]] = d.point_bad[j] ? 1 : 0;
    for (int32_t j = 0; j < d.n_kf_rows; ++j) {
        kf_bad[(size_t)d.kf_idx[j]] = d.kf_bad[j] ? 1 : 0;
        parent[(size_t)d.kf_idx[j]] = d.kf_parent[j];
    }
    for (int32_t k = 0; k < K1; ++k) {
        if (d.kf_order) kf_order[(size_t)k] = d.kf_order[k];
        else if (k >= K0) kf_order[(size_t)k] = k;
    }
    SivoLocalMapTables t;
    t.n_kf = K1; t.n_points = P1;
    t.obs_off = new_off[LMD_OBS].data(); t.obs_kf = new_val[LMD_OBS].data(); t.point_bad = point_bad.data(); t.kf_bad = kf_bad.data();
    t.slot_off = new_off[LMD_SLOT].data(); t.slot_point = new_val[LMD_SLOT].data(); t.covis_off = new_off[LMD_COVIS].data();
    t.covis_kf = new_val[LMD_COVIS].data(); t.child_off = new_off[LMD_CHILD].data(); t.child_kf = new_val[LMD_CHILD].data();
    t.parent = parent.data(); t.kf_order = kf_order.data();
    m->load(t);                                                         // the handle's own copies: the locals above end here
    return SIVO_OK;
}

int sivo_localmap_sizes(sivo_localmap_t m, int64_t out[6]) {
    if (!m) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_sizes", "null handle");
    if (!out) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_sizes", "null out");
    out[0] = m->t.n_kf; out[1] = m->t.n_points;
    localmap_host::totals(*m, out + 2);
    return SIVO_OK;
}

int sivo_localmap_export(sivo_localmap_t m, SivoLocalMapTables *out) {
    if (!m) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_export", "null handle");
    int64_t total[sivo::LMD_TABLES];
    localmap_host::totals(*m, total);
    if (const char *e = sivo::lmd_check_export(m->t.n_kf, m->t.n_points, total, out)) return localmap_host::fail(SIVO_ERR_INVALID_ARGUMENT, "sivo_localmap_export", e);
    const size_t K = (size_t)m->t.n_kf, P = (size_t)m->t.n_points;
    auto down = [](const void *dst, const void *src, size_t bytes) {
        if (bytes) std::memcpy(const_cast<void *>(dst), src, bytes);
    };
    down(out->obs_off, m->obs_off.data(), P ? 8 * (P + 1) : 0); down(out->obs_kf, m->obs_kf.data(), 4 * m->obs_kf.size());
    down(out->point_bad, m->point_bad.data(), P); down(out->kf_bad, m->kf_bad.data(), K);
    down(out->slot_off, m->slot_off.data(), K ? 8 * (K + 1) : 0); down(out->slot_point, m->slot_point.data(), 4 * m->slot_point.size());
    down(out->covis_off, m->covis_off.data(), K ? 8 * (K + 1) : 0); down(out->covis_kf, m->covis_kf.data(), 4 * m->covis_kf.size());
    down(out->child_off, m->child_off.data(), K ? 8 * (K + 1) : 0); down(out->child_kf, m->child_kf.data(), 4 * m->child_kf.size());
    down(out->parent, m->parent.data(), 4 * K); down(out->kf_order, m->kf_order.data(), 4 * K);
    return SIVO_OK;
}

}  // extern "C"
