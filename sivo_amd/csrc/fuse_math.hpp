// fuse_math.hpp — the per-point tests in front of the window query of the two ORBmatcher::Fuse (reference src/orbslam/ORBmatcher.cc:814-852
// with a keyframe's pose, :966-1006 with a Sim3) for one (keyframe, map point) pair, and the argument rules of sivo_fuse_batch; shared by
// the kernel (fuse_batch.hip) and, compiled by g++, by the host programs of the tests.  Every operation stands in the order and the
// precision SIVO::matcher_detail::project_for_fusion evaluates it in (Pose::apply, norm3 and its double dot product; no contraction):
//   * p3Dc = Rcw * p3Dw + tcw: each row summed left to right in float, then + t;
//   * invz = 1 / z: the reference divides in float in the Tcw form and in double (1.0 / z, then narrowed) in the Scw form; both are the
//     correctly rounded float quotient (a double quotient of two floats rounds to float without a second error: 53 >= 2 * 24 + 2), so
//     one float division serves both;
//   * u = fx * (x * invz) + cx, v likewise; KeyFrame::IsInImage with >= min and < max; ur = u - bf * invz;
//   * PO = p3Dw - Ow with the camera centre AS GIVEN (GetCameraCenter() in the Tcw form, -Rcw' tcw in the Scw form: the caller's);
//     cv::norm(PO) and PO.dot(Pn) sum in double; the angle test compares that double with 0.5 * (double)dist3D;
//   * the level is frustum_math.hpp's fr_level over the host-made threshold table of fr_level_table (no logarithm on the device;
//     the KeyFrame and the Frame form of MapPoint::PredictScale are one expression, MapPoint.cc:423-453).
// The two forms differ behind these tests only (the chi-square gates of :878-899 exist in the Tcw form alone): `scw_variant` is read
// by the candidate scan, not here.
#pragma once
#include "frustum_math.hpp"

namespace sivo {

struct FuCamera {              // SivoFuseCamera with the level thresholds derived from it once per call
    SivoFuseCamera c;
    float T[15];               // nlevels - 1 of them
};

struct FuResult {
    float u, v, ur;
    int32_t level;
};

enum { SIVO_FUSE_REACHED = 255 };         // not a status of the ABI: the pair goes on to the window query

// ORBmatcher.cc:814-849 / :966-1003 for one point; the SIVO_FUSE_* of the `continue` it took, or SIVO_FUSE_REACHED with `o` written.
SIVO_HD uint8_t fu_point(const FuCamera &fc, const float *X, const float *Pn, float min_dist, float max_dist, FuResult &o) {
    const SivoFuseCamera &c = fc.c;
    float Pc[3];
    for (int r = 0; r < 3; ++r) {
        float s = c.Rcw[3 * r] * X[0];
        s = s + c.Rcw[3 * r + 1] * X[1];
        s = s + c.Rcw[3 * r + 2] * X[2];
        Pc[r] = s + c.tcw[r];
    }
    if (Pc[2] < 0.0f) return SIVO_FUSE_BEHIND;                                            // :818
    const float invz = 1.0f / Pc[2];
    const float x = Pc[0] * invz, y = Pc[1] * invz;
    const float u = c.fx * x + c.cx;
    const float v = c.fy * y + c.cy;
    if (!(u >= c.min_x && u < c.max_x && v >= c.min_y && v < c.max_y)) return SIVO_FUSE_IMAGE;   // :829, KeyFrame.cc:638-640
    const float ur = u - c.bf * invz;
    const float PO[3] = {X[0] - c.Ow[0], X[1] - c.Ow[1], X[2] - c.Ow[2]};
    double s2 = (double)PO[0] * (double)PO[0];
    s2 += (double)PO[1] * (double)PO[1];
    s2 += (double)PO[2] * (double)PO[2];
    const float dist = (float)sqrt(s2);
    if (dist < 0.8f * min_dist || dist > 1.2f * max_dist) return SIVO_FUSE_DISTANCE;     // :840, MapPoint.cc:413-421
    double dot = (double)PO[0] * (double)Pn[0];
    dot += (double)PO[1] * (double)Pn[1];
    dot += (double)PO[2] * (double)Pn[2];
    if (dot < 0.5 * (double)dist) return SIVO_FUSE_ANGLE;                                 // :846
    const float ratio = max_dist / dist;                                                  // MapPoint.cc:427
    o.u = u; o.v = v; o.ur = ur;
    o.level = fr_level(ratio, fc.T, c.nlevels);
    return SIVO_FUSE_REACHED;
}

// ---- host only ----
inline void fu_camera(const SivoFuseCamera &c, FuCamera &fc) {          // after fu_check_batch: nlevels and the logarithm are in range
    fc.c = c;
    for (int k = 0; k < 15; ++k) fc.T[k] = 0.0f;
    fr_level_table(c.log_scale_factor, c.nlevels, fc.T);
}

// The argument rules of sivo_fuse_batch, in the order the header lists them; nullptr when the call may go on.  FrameT: anything with
// `device` and `nlevels` (the library's sivo_mframe, the host stand-in of the tests).
template <class FrameT>
const char *fu_check_batch(FrameT *const *kfs, const SivoFuseCamera *cams, int n_kf, int n_mp, const float *pos, const float *normal,
                           const float *min_dist, const float *max_dist, const uint8_t *mp_desc, const int32_t *best_idx,
                           const int32_t *best_dist, const uint8_t *status) {
    if (n_kf < 0 || n_mp < 0) return "negative count";
    if (n_kf > 0 && !kfs) return "null frame array";
    if (n_kf > 0 && !cams) return "null camera array";
    if (n_mp > 0 && !(pos && normal && min_dist && max_dist && mp_desc)) return "null point array";
    if (n_kf > 0 && n_mp > 0 && !(best_idx && best_dist && status)) return "null output";
    if ((int64_t)n_kf * (int64_t)n_mp > ((int64_t)1 << 24)) return "more than 2^24 pairs";
    for (int k = 0; k < n_kf; ++k) {
        if (!kfs[k]) return "null frame";
        if (kfs[k]->device != kfs[0]->device) return "frames on different devices";
        if (cams[k].nlevels < 1 || cams[k].nlevels > 16) return "nlevels outside 1 .. 16";
        if (cams[k].nlevels > kfs[k]->nlevels) return "nlevels above the frame's";
        if (!(cams[k].log_scale_factor > 0.0f)) return "log_scale_factor is not positive";
    }
    return nullptr;
}

}  // namespace sivo
