// fuse_batch_host_capi.hpp — sivo_fuse_batch of include/sivo_hip.h over the HOST build of the kernel's per-pair arithmetic
// (sivo_amd/csrc/fuse_math.hpp), with the argument rules of the library (fu_check_batch of that header) and the results stored as
// fuse_batch.hip stores them; and the three entry points the single-keyframe ORBmatcher::Fuse members call (sivo_mframe_create,
// sivo_mframe_destroy, sivo_fuse), so that the adapter's program can run the loop of single calls beside the batch.  The candidate scan
// is a plain sequential loop over Frame::GetFeaturesInArea's order in place of the wave, over the grid, the window and the chi-square
// gate of sivo_amd/csrc/grid_math.hpp (the functions the kernels run): no library, no device, so the programs that
// include it (tests/fuse_batch_prog.cpp, tests/fuse_batch_adapter_prog.cpp) can run under the sanitizers.
#pragma once
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fuse_math.hpp"
#include "grid_math.hpp"

// A frame handle on the host: copies of the arrays and the 64 x 48 grid in mGrid[ix][iy] order (Frame.cc:205-221, :392-404).
struct sivo_mframe {
    int device = 0, n = 0, nlevels = 0;
    float min_x = 0, max_x = 0, min_y = 0, max_y = 0, inv_w = 0, inv_h = 0;
    std::vector<SivoKeyPoint> keys;
    std::vector<float> u_right, scale, inv_sigma2;
    std::vector<uint8_t> desc;
    std::vector<int32_t> cell_off, cell_idx;
};

namespace fuse_batch_host {
enum { ROWS = SIVO_GRID_ROWS, TH_LOW = 50 };
inline std::string &error() { static std::string e; return e; }
inline int fail(const char *where, const char *what) { error() = std::string(where) + ": " + what; return SIVO_ERR_INVALID_ARGUMENT; }
struct Counters { long batch = 0, single = 0, frames_alive = 0; };
inline Counters &counters() { static Counters c; return c; }        // how many entry-point calls were made

inline void features_in_area(const sivo_mframe &F, float x, float y, float r, std::vector<int32_t> &out) {
    out.clear();
    int c0, c1, r0, r1;
    if (!sivo::grid_window(F.min_x, F.min_y, F.inv_w, F.inv_h, x, y, r, c0, c1, r0, r1)) return;
    for (int ix = c0; ix <= c1; ++ix)
        for (int iy = r0; iy <= r1; ++iy)
            for (int j = F.cell_off[(size_t)(ix * ROWS + iy)]; j < F.cell_off[(size_t)(ix * ROWS + iy + 1)]; ++j) {
                const SivoKeyPoint &kp = F.keys[(size_t)F.cell_idx[(size_t)j]];
                if (sivo::in_window(kp.x, kp.y, x, y, r)) out.push_back(F.cell_idx[(size_t)j]);
            }
}

inline int hamming(const uint8_t *a, const uint8_t *b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

// the candidate loop of ORBmatcher.cc:865-909 / :1019-1036 for one projected point; `seen`: the window held a key
inline void scan(const sivo_mframe &F, float u, float v, float ur, int level, const uint8_t *desc, float th, int scw_variant, int &best,
                 int &best_dist, bool &seen) {
    std::vector<int32_t> idx;
    features_in_area(F, u, v, th * F.scale[(size_t)level], idx);
    seen = !idx.empty();
    best = -1;
    best_dist = scw_variant ? INT_MAX : 256;
    for (int32_t i : idx) {
        const SivoKeyPoint &kp = F.keys[(size_t)i];
        if (kp.octave < level - 1 || kp.octave > level) continue;
        if (!scw_variant) {
            const float kur = F.u_right.empty() ? -1.0f : F.u_right[(size_t)i];
            if (!sivo::fuse_chi2_gate(u - kp.x, v - kp.y, kur >= 0, ur - kur, F.inv_sigma2[(size_t)kp.octave])) continue;
        }
        const int d = hamming(desc, F.desc.data() + 32 * (size_t)i);
        if (d < best_dist) { best_dist = d; best = i; }
    }
    if (best_dist > TH_LOW) best = -1;
    if (scw_variant && best_dist == 256) best_dist = INT_MAX;          // (as sivo_fuse reports a scan that compared nothing)
}
}  // namespace fuse_batch_host

extern "C" {

const char *sivo_last_error(void) { return fuse_batch_host::error().c_str(); }

int sivo_mframe_create(const SivoKeyPoint *keys, int n, const float *u_right, const uint8_t *descriptors, float min_x, float max_x,
                       float min_y, float max_y, const float *scale_factors, const float *, const float *inv_level_sigma2, int nlevels,
                       int device, sivo_mframe_t *out) {
    using namespace fuse_batch_host;
    sivo_mframe *F = new sivo_mframe;
    F->device = device < 0 ? 0 : device; F->n = n; F->nlevels = nlevels;
    F->min_x = min_x; F->max_x = max_x; F->min_y = min_y; F->max_y = max_y;
    F->inv_w = (float)SIVO_GRID_COLS / (max_x - min_x);
    F->inv_h = (float)SIVO_GRID_ROWS / (max_y - min_y);
    if (n) F->keys.assign(keys, keys + n);
    if (u_right && n) F->u_right.assign(u_right, u_right + n);
    if (n) F->desc.assign(descriptors, descriptors + 32 * (size_t)n);
    F->scale.assign(scale_factors, scale_factors + nlevels);
    F->inv_sigma2.assign(inv_level_sigma2, inv_level_sigma2 + nlevels);
    sivo::grid_build(keys, n, min_x, min_y, F->inv_w, F->inv_h, F->cell_off, F->cell_idx);
    ++counters().frames_alive;
    *out = F;
    return SIVO_OK;
}

int sivo_mframe_destroy(sivo_mframe_t h) {
    if (h) { delete h; --fuse_batch_host::counters().frames_alive; }
    return SIVO_OK;
}

int sivo_fuse(sivo_mframe_t kf, int n_mp, const uint8_t *valid, const float *u, const float *v, const float *ur, const int32_t *pred_level,
              const uint8_t *mp_desc, float th, int scw_variant, int32_t *best_idx, int32_t *best_dist, int *n_fused) {
    using namespace fuse_batch_host;
    ++counters().single;
    int n = 0;
    for (int i = 0; i < n_mp; ++i) {
        int best = -1, dist = scw_variant ? INT_MAX : 256;
        bool seen = false;
        if (valid[i]) scan(*kf, u[i], v[i], ur ? ur[i] : 0.0f, pred_level[i], mp_desc + 32 * (size_t)i, th, scw_variant, best, dist, seen);
        best_idx[i] = best;
        if (best_dist) best_dist[i] = dist;
        n += best >= 0;
    }
    if (n_fused) *n_fused = n;
    return SIVO_OK;
}

int sivo_fuse_batch(const sivo_mframe_t *kfs, const SivoFuseCamera *cams, int n_kf, int n_mp, const float *pos, const float *normal,
                    const float *min_dist, const float *max_dist, const uint8_t *mp_desc, const uint8_t *skip_point, const uint8_t *skip_pair,
                    float th, int32_t *best_idx, int32_t *best_dist, uint8_t *status, float *u, float *v, float *ur, int32_t *level) {
    using namespace fuse_batch_host;
    ++counters().batch;
    if (const char *e = sivo::fu_check_batch(kfs, cams, n_kf, n_mp, pos, normal, min_dist, max_dist, mp_desc, best_idx, best_dist, status))
        return fail("sivo_fuse_batch", e);
    for (int k = 0; k < n_kf; ++k) {
        sivo::FuCamera cam;
        sivo::fu_camera(cams[k], cam);
        const int none = cams[k].scw_variant ? INT_MAX : 256;
        for (int i = 0; i < n_mp; ++i) {
            const size_t pair = (size_t)k * (size_t)n_mp + (size_t)i;
            uint8_t st = SIVO_FUSE_SKIPPED;
            sivo::FuResult o;
            if (!(skip_point && skip_point[i]) && !(skip_pair && skip_pair[pair]))
                st = sivo::fu_point(cam, pos + 3 * (size_t)i, normal + 3 * (size_t)i, min_dist[i], max_dist[i], o);
            if (st != sivo::SIVO_FUSE_REACHED) { best_idx[pair] = -1; best_dist[pair] = none; status[pair] = st; continue; }
            int best, dist;
            bool seen;
            scan(*kfs[k], o.u, o.v, o.ur, o.level, mp_desc + 32 * (size_t)i, th, cams[k].scw_variant, best, dist, seen);
            best_idx[pair] = best; best_dist[pair] = dist;
            status[pair] = best >= 0 ? SIVO_FUSE_MATCHED : seen ? SIVO_FUSE_TOO_FAR : SIVO_FUSE_NO_CANDIDATE;
            if (u) u[pair] = o.u;
            if (v) v[pair] = o.v;
            if (ur) ur[pair] = o.ur;
            if (level) level[pair] = o.level;
        }
    }
    return SIVO_OK;
}

}  // extern "C"
