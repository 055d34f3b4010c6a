// frustum_math.hpp — Frame::isInFrustum (reference src/orbslam/Frame.cc:267-324) with MapPoint::PredictScale (MapPoint.cc:439-453) for one
// map point, and the SivoSearchQuery that ORBmatcher::SearchByProjection(Frame &, const vector<MapPoint *> &, th) (ORBmatcher.cc:44-127)
// makes of a point in view; shared by the kernels (frustum.hip, search.hip) and, compiled by g++, by the host programs of the tests.
// Every operation stands in the order and the precision of the cv::Mat expressions the reference evaluates (no contraction):
//   * Pc = mRcw * P + mtcw is gemm's small-matrix path: each row summed left to right in float, then + t (matcher_detail::Pose::apply);
//   * mOw = -mRcw.t() * mtcw goes through the general kernel: products and sum in double, rounded once (Pose::centre);
//   * cv::norm(PO) and PO.dot(Pn) sum in double; PO.dot(Pn) / dist divides that double by the float dist.
// The level.  PredictScale is ceil(logf(maxDist / dist) / mfLogScaleFactor) clamped to [0, nlevels - 1]: the one call into libm, and a
// device logf need not agree with the host's to the last bit where the ratio stands at scaleFactor^k.  The device therefore takes no
// logarithm: the host finds, by bisection over the bit patterns of the positive floats with ITS logf (the one the reference calls), the
// largest float T[k] whose level is <= k, for k = 0 .. nlevels - 2; logf is monotone, so the level of a ratio is the number of k with
// ratio > T[k] (a NaN ratio counts none: level 0, where the reference's clamp of the converted NaN also ends).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/sivo_hip.h"

#ifndef SIVO_HD
#ifdef __HIPCC__
#define SIVO_HD __host__ __device__ inline
#else
#define SIVO_HD inline
#endif
#endif

namespace sivo {

struct FrCamera {              // SivoFrustum with what is derived from it once per call
    SivoFrustum f;
    float Ow[3];               // mOw
    float T[15];               // level thresholds, nlevels - 1 of them
};

struct FrResult {
    float u, v, ur, view_cos;  // mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos
    int32_t level;             // mnTrackScaleLevel
};

// mOw = -mRcw.t() * mtcw
SIVO_HD void fr_centre(const float *R, const float *t, float *Ow) {
    for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (int r = 0; r < 3; ++r) s += (double)R[3 * r + c] * (double)t[r];
        Ow[c] = (float)(-s);
    }
}

// the number of thresholds below the ratio
SIVO_HD int fr_level(float ratio, const float *T, int nlevels) {
    int level = 0;
    for (int k = 0; k < nlevels - 1; ++k) level += ratio > T[k] ? 1 : 0;
    return level;
}

// Frame.cc:267-324 for one point; the SIVO_FRUSTUM_* of the exit.  `o` is written only for a point in view.
SIVO_HD uint8_t fr_point(const FrCamera &c, const float *X, const float *Pn, float min_dist, float max_dist, FrResult &o) {
    const SivoFrustum &f = c.f;
    float Pc[3];
    for (int r = 0; r < 3; ++r) {
        float s = f.Rcw[3 * r] * X[0];
        s = s + f.Rcw[3 * r + 1] * X[1];
        s = s + f.Rcw[3 * r + 2] * X[2];
        Pc[r] = s + f.tcw[r];
    }
    if (Pc[2] < 0.0f) return SIVO_FRUSTUM_BEHIND;                                      // :280
    const float invz = 1.0f / Pc[2];
    const float u = f.fx * Pc[0] * invz + f.cx;
    const float v = f.fy * Pc[1] * invz + f.cy;
    if (u < f.min_x || u > f.max_x) return SIVO_FRUSTUM_U;                             // :288
    if (v < f.min_y || v > f.max_y) return SIVO_FRUSTUM_V;                             // :290
    const float PO[3] = {X[0] - c.Ow[0], X[1] - c.Ow[1], X[2] - c.Ow[2]};
    double s2 = (double)PO[0] * (double)PO[0];
    s2 += (double)PO[1] * (double)PO[1];
    s2 += (double)PO[2] * (double)PO[2];
    const float dist = (float)sqrt(s2);
    if (dist < 0.8f * min_dist || dist > 1.2f * max_dist) return SIVO_FRUSTUM_DISTANCE;   // :299, MapPoint.cc:413-421
    double dot = (double)PO[0] * (double)Pn[0];
    dot += (double)PO[1] * (double)Pn[1];
    dot += (double)PO[2] * (double)Pn[2];
    const float view_cos = (float)(dot / (double)dist);
    if (view_cos < f.cos_limit) return SIVO_FRUSTUM_ANGLE;                             // :308
    const float ratio = max_dist / dist;                                               // MapPoint.cc:443
    o.u = u; o.v = v; o.ur = u - f.bf * invz; o.view_cos = view_cos;
    o.level = fr_level(ratio, c.T, f.nlevels);
    return SIVO_FRUSTUM_IN_VIEW;
}

// The query of a point in view (ORBmatcher.cc:57-76): the window RadiusByViewingCos (:129-134) times th when th != 1, times the
// predicted level's scale; octaves [level - 1, level]; the same length gates |ur - mvRight[k]|.  scale: the frame's mvScaleFactors.
SIVO_HD void fr_query(const FrResult &o, float th, const float *scale, int32_t obs, SivoSearchQuery &q) {
    float r = o.view_cos > 0.998 ? 2.5f : 4.0f;
    if (th != 1.0) r *= th;
    q.u = o.u; q.v = o.v;
    q.radius = r * scale[o.level];
    q.lvl_lo = o.level - 1; q.lvl_hi = o.level;
    q.ur = o.ur; q.gate = r * scale[o.level];
    q.angle = 0.0f;
    q.flags = SIVO_Q_VALID | (obs > 0 ? SIVO_Q_BLOCKS : 0);
}

SIVO_HD void fr_no_query(SivoSearchQuery &q) {
    q.u = 0.0f; q.v = 0.0f; q.radius = 0.0f; q.lvl_lo = 0; q.lvl_hi = 0; q.ur = 0.0f; q.gate = 0.0f; q.angle = 0.0f; q.flags = 0;
}

// ---- host only ----
// MapPoint.cc:446-450 as written: the level of a ratio through the host's logf
inline int fr_level_direct(float ratio, float log_scale_factor, int nlevels) {
    const float c = ceilf(logf(ratio) / log_scale_factor);
    return c != c ? 0 : c < 0.0f ? 0 : c >= (float)nlevels ? nlevels - 1 : (int)c;
}

// T[k], k = 0 .. nlevels - 2: the largest float whose level by the direct expression (before the clamp) is <= k.  The bit patterns of the
// positive floats ascend with their values: 31 halvings between the smallest subnormal (its level is far below 0) and +inf (above
// every k).  log_scale_factor must be positive.
inline void fr_level_table(float log_scale_factor, int nlevels, float *T) {
    for (int k = 0; k < nlevels - 1; ++k) {
        uint32_t lo = 1u, hi = 0x7F800000u;                       // level(lo) <= k < level(hi)
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            float x;
            memcpy(&x, &mid, 4);
            if (ceilf(logf(x) / log_scale_factor) <= (float)k) lo = mid;
            else hi = mid;
        }
        memcpy(&T[k], &lo, 4);
    }
}

// nlevels in [1, 16] and a positive logarithm (a scale factor above 1): what the table needs
inline bool fr_camera(const SivoFrustum &f, FrCamera &c) {
    if (f.nlevels < 1 || f.nlevels > 16 || !(f.log_scale_factor > 0.0f)) return false;
    c.f = f;
    fr_centre(f.Rcw, f.tcw, c.Ow);
    for (int k = 0; k < 15; ++k) c.T[k] = 0.0f;
    fr_level_table(f.log_scale_factor, f.nlevels, c.T);
    return true;
}

}  // namespace sivo
