// local_mapping_host_capi.hpp — sivo_triangulate and sivo_mappoint_refresh of include/sivo_hip.h over the HOST build of the kernels' arithmetic
// (sivo_amd/csrc/triangulate_math.hpp, mappoint_math.hpp: what tests/local_mapping_prog.cpp runs), with the results stored as
// sivo_amd/csrc/triangulate.hip and mappoint.hip store them (every NaN as 0x7FC00000, a flagged point's entries left as the caller had
// them).  tests/local_mapping_adapter_prog.cpp built with -DSIVO_LM_ON_HOST includes it, so that its definitions stand in front of the
// library's and SIVO::CreateNewMapPoints / TriangulateMatches / RefreshMapPoints (sivo_amd/api/orbslam/LocalMappingAdapter.h) run
// without a device: tests/test_pin_local_mapping.py holds the adapter's walk over the neighbours to the reference's own there.
#pragma once
#include <cstring>

#include "mappoint_math.hpp"
#include "triangulate_math.hpp"

extern "C" {

int sivo_triangulate(SivoTriProblem *P) {
    if (!P || P->n < 0 || (P->n > 0 && (!P->matches || !P->status || !P->wP || !P->detected_class))) return SIVO_ERR_INVALID_ARGUMENT;
    if (P->kf1.nlevels < 1 || P->kf1.nlevels > 16 || P->kf2.nlevels < 1 || P->kf2.nlevels > 16) return SIVO_ERR_INVALID_ARGUMENT;
    for (int32_t i = 0; i < P->n; ++i) {
        const SivoTriMatch &m = P->matches[i];
        if (m.octave1 < 0 || m.octave1 >= P->kf1.nlevels || m.octave2 < 0 || m.octave2 >= P->kf2.nlevels) return SIVO_ERR_INVALID_ARGUMENT;
    }
    for (int32_t i = 0; i < P->n; ++i) {
        sivo::TrResult o;
        sivo::tr_match(P->kf1, P->kf2, P->ratio_factor, P->state_cov, P->th_confidence, P->th_entropy, P->matches[i], o);
        P->status[i] = o.status;
        P->detected_class[i] = o.cls;
        for (int c = 0; c < 3; ++c) {
            const uint32_t bits = sivo::tr_float_bits(o.wP[c]);
            std::memcpy(&P->wP[3 * i + c], &bits, 4);
        }
    }
    return SIVO_OK;
}

int sivo_mappoint_refresh(int np, const int64_t *desc_off, const uint8_t *desc, const int64_t *obs_off, const float *obs_ow, const float *pos,
                          const float *ref_ow, const float *level_scale, const float *last_scale, int32_t *best_idx, float *max_dist,
                          float *min_dist, float *normal, uint8_t *flags) {
    if (np < 0) return SIVO_ERR_INVALID_ARGUMENT;
    for (int p = 0; p < np; ++p) {
        const int64_t N = desc_off[p + 1] - desc_off[p], M = obs_off[p + 1] - obs_off[p];
        if (N < 0 || M < 0) return SIVO_ERR_INVALID_ARGUMENT;
        if (M == 0) { flags[p] = SIVO_MP_NO_OBSERVATION | SIVO_MP_NO_DESCRIPTOR; continue; }
        flags[p] = N > 0 ? 0 : SIVO_MP_NO_DESCRIPTOR;
        if (N > 0) {
            std::vector<uint64_t> d(4 * (size_t)N);                  // (the kernel reads the descriptors as aligned 64-bit words)
            std::memcpy(d.data(), desc + 32 * desc_off[p], 32 * (size_t)N);
            int best = 0x7FFFFFFF;
            for (int64_t i = 0; i < N; ++i) {
                const int med = sivo::mp_row_median(d.data(), N, i);
                if (med < best) { best = med; best_idx[p] = (int32_t)i; }      // the first row with the smallest median
            }
        }
        float o[5];
        sivo::mp_normal_depth(pos + 3 * p, obs_ow + 3 * obs_off[p], M, ref_ow + 3 * p, level_scale[p], last_scale[p], o);
        const float *src[5] = {&o[0], &o[1], &o[2], &o[3], &o[4]};
        float *dst[5] = {max_dist + p, min_dist + p, normal + 3 * p, normal + 3 * p + 1, normal + 3 * p + 2};
        for (int c = 0; c < 5; ++c) {
            const uint32_t bits = sivo::tr_float_bits(*src[c]);
            std::memcpy(dst[c], &bits, 4);
        }
    }
    return SIVO_OK;
}

}  // extern "C"
