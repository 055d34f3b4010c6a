// mappoint_math.hpp — the arithmetic of MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (reference
// src/orbslam/MapPoint.cc:284-347, :368-411) for one map point, shared by the kernel (mappoint.hip) and, compiled by g++, by the host
// program of the restatement tests.
//   * The median of row i of the N x N Hamming matrix is the element k = (int)(0.5 (N - 1)) of the sorted row (:333-335): the smallest
//     value v with #{j : d(i, j) <= v} > k.  Distances are integers in [0, 256]: nine halvings of that interval find v, each counting
//     over the row — rank selection, nothing is sorted and no row is stored, so N has no upper limit.
//   * The normal is the running float sum of normali / cv::norm(normali) in observation order (:391-397): the norm in double, the
//     quotient a convertTo with the factor 1 / norm narrowed to float (api/compat/cv_min.hpp), the sum and normal / n likewise.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef SIVO_HD
#ifdef __HIPCC__
#define SIVO_HD __host__ __device__ inline
#else
#define SIVO_HD inline
#endif
#endif

namespace sivo {

// ORBmatcher::DescriptorDistance on two 32-byte descriptors read as 4 x u64 (popcounts add: the word size does not matter)
SIVO_HD int mp_distance(const uint64_t *a, const uint64_t *b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __popcll(a[0] ^ b[0]) + __popcll(a[1] ^ b[1]) + __popcll(a[2] ^ b[2]) + __popcll(a[3] ^ b[3]);
#else
    return __builtin_popcountll(a[0] ^ b[0]) + __builtin_popcountll(a[1] ^ b[1]) + __builtin_popcountll(a[2] ^ b[2]) +
           __builtin_popcountll(a[3] ^ b[3]);
#endif
}

// vDists[0.5 * (N - 1)] of the sorted row i (:333-335); desc: N descriptors of 4 x u64
SIVO_HD int mp_row_median(const uint64_t *desc, int64_t N, int64_t i) {
    const int64_t k = (int64_t)(0.5 * (double)(N - 1));
    const uint64_t mine[4] = {desc[4 * i], desc[4 * i + 1], desc[4 * i + 2], desc[4 * i + 3]};
    int lo = 0, hi = 256;
    for (int step = 0; step < 9; ++step) {              // 257 candidates: nine halvings
        const int mid = (lo + hi) >> 1;
        int64_t count = 0;
        for (int64_t j = 0; j < N; ++j) count += mp_distance(mine, desc + 4 * j) <= mid;
        if (lo < hi) {
            if (count > k) hi = mid;
            else lo = mid + 1;
        }
    }
    return lo;
}

// :389-410.  ow: the camera centres of the M >= 1 observations; out: max, min, normal[3]
SIVO_HD void mp_normal_depth(const float *pos, const float *ow, int64_t M, const float *ref_ow, float level_scale, float last_scale, float *out) {
    float normal[3] = {0.0f, 0.0f, 0.0f};
    for (int64_t j = 0; j < M; ++j) {
        const float d[3] = {pos[0] - ow[3 * j], pos[1] - ow[3 * j + 1], pos[2] - ow[3 * j + 2]};
        double s = 0.0;
        s += (double)d[0] * (double)d[0]; s += (double)d[1] * (double)d[1]; s += (double)d[2] * (double)d[2];
        const float f = (float)(1.0 / sqrt(s));
        normal[0] = normal[0] + d[0] * f; normal[1] = normal[1] + d[1] * f; normal[2] = normal[2] + d[2] * f;
    }
    const float pc[3] = {pos[0] - ref_ow[0], pos[1] - ref_ow[1], pos[2] - ref_ow[2]};
    double s = 0.0;
    s += (double)pc[0] * (double)pc[0]; s += (double)pc[1] * (double)pc[1]; s += (double)pc[2] * (double)pc[2];
    const float dist = (float)sqrt(s);
    out[0] = dist * level_scale;
    out[1] = out[0] / last_scale;
    const float fn = (float)(1.0 / (double)M);          // normal / n: n an int
    out[2] = normal[0] * fn; out[3] = normal[1] * fn; out[4] = normal[2] * fn;
}

}  // namespace sivo
