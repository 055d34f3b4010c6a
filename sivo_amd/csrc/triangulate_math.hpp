// triangulate_math.hpp — one match of LocalMapping::CreateNewMapPoints (reference src/orbslam/LocalMapping.cc:277-470), operation for
// operation under the float rules of OpenCV 3.x that api/compat/cv_min.hpp states:
//   * A * B (+ C) with no transposed operand and an inner dimension of 3 is gemm's small-matrix path: the dot product accumulated left
//     to right in float, then (float)((double)t * alpha + c)                                                           (tr_gemm3);
//   * Mat::dot and cv::norm accumulate in double                                                                      (tr_dot3);
//   * s * A, A / s are convertTo with the factor narrowed to float; s * A - B is a * (float)s - b.
// Two pieces are restated, neither pinned (OpenCV is absent: DESIGN 3.6e):
//   * cv::SVD::compute(A) on the 4 x 4 float A, of which only vt.row(3) is used  ->  the eigenvector of the smallest eigenvalue of A'A,
//     formed in double from the float A, by the cyclic Jacobi of sim3_ransac.hip (the same rotation, the pairs in the order (0,1) (0,2)
//     (0,3) (1,2) (1,3) (2,3), TR_SWEEPS sweeps, a rotation skipped on an exact-zero entry), ties to the lowest index, rounded to float.
//     Its sign cancels in wP / w;
//   * cos(2 * atan2(mb / 2, depth)), whose overload the source leaves open  ->  (d^2 - a^2) / (d^2 + a^2) in double from the float
//     a = mb / 2 and d = depth, rounded to float.
// Only + - * / sqrt, comparisons and float / double conversions, each correctly rounded without contraction; the log2 of the gate
// (gate_math.hpp) is the one exception.  tests/triangulate_restatement.py restates this file in numpy and is compared bit for bit, with
// the device and with this header compiled by g++ for the host.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/sivo_hip.h"
#include "gate_math.hpp"

namespace sivo {

constexpr int TR_SWEEPS = 8;

struct TrResult {
    uint8_t status, cls;
    float wP[3];
};

SIVO_HD float tr_gemm3(float a0, float a1, float a2, float b0, float b1, float b2, double c) {
    float t = a0 * b0;
    t = t + a1 * b1;
    t = t + a2 * b2;
    return (float)((double)t * 1.0 + c);
}
SIVO_HD double tr_dot3(const float *a, const float *b) {
    double s = 0.0;
    s += (double)a[0] * (double)b[0];
    s += (double)a[1] * (double)b[1];
    s += (double)a[2] * (double)b[2];
    return s;
}
// cos(2 atan2(mb / 2, depth)) (:308-312), restated
SIVO_HD float tr_cos_stereo(float mb, float depth) {
    const double a = (double)(mb / 2), d = (double)depth;
    return (float)((d * d - a * a) / (d * d + a * a));
}

template <int P, int Q>
SIVO_HD void tr_jacobi_rot(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq != 0.0) {          // (a NaN enters: it propagates as every other value does)
        const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0);
        const double s = t * c;
        A[P][P] = A[P][P] - t * apq;
        A[Q][Q] = A[Q][Q] + t * apq;
        A[P][Q] = 0.0; A[Q][P] = 0.0;
        for (int r = 0; r < 4; ++r) {
            if (r == P || r == Q) continue;
            const double arp = A[r][P], arq = A[r][Q];
            A[r][P] = c * arp - s * arq; A[P][r] = A[r][P];
            A[r][Q] = s * arp + c * arq; A[Q][r] = A[r][Q];
        }
        for (int r = 0; r < 4; ++r) {
            const double vrp = V[r][P], vrq = V[r][Q];
            V[r][P] = c * vrp - s * vrq;
            V[r][Q] = s * vrp + c * vrq;
        }
    }
}

// vt.row(3) of cv::SVD::compute(A) (:327-331), restated: e = the null vector of the float A, as floats
SIVO_HD void tr_null_vector(const float (&Af)[4][4], float (&e)[4]) {
    double A[4][4], V[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += (double)Af[k][i] * (double)Af[k][j];
            A[i][j] = s;
            V[i][j] = i == j ? 1.0 : 0.0;
        }
#ifdef __HIPCC__
#pragma unroll 1
#endif
    for (int sweep = 0; sweep < TR_SWEEPS; ++sweep) {
        tr_jacobi_rot<0, 1>(A, V); tr_jacobi_rot<0, 2>(A, V); tr_jacobi_rot<0, 3>(A, V);
        tr_jacobi_rot<1, 2>(A, V); tr_jacobi_rot<1, 3>(A, V); tr_jacobi_rot<2, 3>(A, V);
    }
    double best = A[0][0], v[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
    if (A[1][1] < best) { best = A[1][1]; v[0] = V[0][1]; v[1] = V[1][1]; v[2] = V[2][1]; v[3] = V[3][1]; }
    if (A[2][2] < best) { best = A[2][2]; v[0] = V[0][2]; v[1] = V[1][2]; v[2] = V[2][2]; v[3] = V[3][2]; }
    if (A[3][3] < best) { best = A[3][3]; v[0] = V[0][3]; v[1] = V[1][3]; v[2] = V[2][3]; v[3] = V[3][3]; }
    for (int i = 0; i < 4; ++i) e[i] = (float)v[i];
}

// the reprojection test of one keyframe (:364-392 / :394-425); `mbf` is the CURRENT keyframe's in both (:383, :414)
SIVO_HD bool tr_reproj_fails(const SivoTriKeyFrame &k, const float *wP, float z, bool stereo, float px, float py, float pr, float sigma2, float mbf) {
    const float x = (float)(tr_dot3(k.Rcw, wP) + (double)k.tcw[0]);
    const float y = (float)(tr_dot3(k.Rcw + 3, wP) + (double)k.tcw[1]);
    const float invz = 1.0f / z;
    const float u = k.fx * x * invz + k.cx;
    const float v = k.fy * y * invz + k.cy;
    const float ex = u - px, ey = v - py;
    if (!stereo) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    const float ur = u - mbf * invz;
    const float er = ur - pr;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

// KeyFrame::UnprojectStereo (KeyFrame.cc:642-656): Twc.R * x3Dc + Twc.t, one gemm
SIVO_HD void tr_unproject(const SivoTriKeyFrame &k, float u, float v, float z, float *wP) {
    const float x = (u - k.cx) * z * k.invfx;
    const float y = (v - k.cy) * z * k.invfy;
    for (int i = 0; i < 3; ++i) wP[i] = tr_gemm3(k.Twc[4 * i], k.Twc[4 * i + 1], k.Twc[4 * i + 2], x, y, z, (double)k.Twc[4 * i + 3] * 1.0);
}

// the octaves have been checked by the host: 0 <= octave < nlevels <= 16
SIVO_HD void tr_match(const SivoTriKeyFrame &k1, const SivoTriKeyFrame &k2, float ratio_factor, const double *Sx, double th_conf, double th_ent,
                      const SivoTriMatch &m, TrResult &o) {
    o.status = SIVO_TRI_LOW_PARALLAX; o.cls = 255;
    float wP[3] = {0.0f, 0.0f, 0.0f};
    o.wP[0] = 0.0f; o.wP[1] = 0.0f; o.wP[2] = 0.0f;
    const bool stereo1 = m.r1 >= 0, stereo2 = m.r2 >= 0;
    // :289-300
    const float xn1[3] = {(m.x1 - k1.cx) * k1.invfx, (m.y1 - k1.cy) * k1.invfy, 1.0f};
    const float xn2[3] = {(m.x2 - k2.cx) * k2.invfx, (m.y2 - k2.cy) * k2.invfy, 1.0f};
    float ray1[3], ray2[3];
    for (int i = 0; i < 3; ++i) {          // Rwc = Rcw.t() materialised: Rwc(i, k) = Rcw(k, i)
        ray1[i] = tr_gemm3(k1.Rcw[i], k1.Rcw[3 + i], k1.Rcw[6 + i], xn1[0], xn1[1], xn1[2], 0.0);
        ray2[i] = tr_gemm3(k2.Rcw[i], k2.Rcw[3 + i], k2.Rcw[6 + i], xn2[0], xn2[1], xn2[2], 0.0);
    }
    const float cos_rays = (float)(tr_dot3(ray1, ray2) / (sqrt(tr_dot3(ray1, ray1)) * sqrt(tr_dot3(ray2, ray2))));
    const float cos_stereo0 = cos_rays + 1;
    float cos_stereo1 = cos_stereo0, cos_stereo2 = cos_stereo0;
    if (stereo1) cos_stereo1 = tr_cos_stereo(k1.mb, m.depth1);
    else if (stereo2) cos_stereo2 = tr_cos_stereo(k2.mb, m.depth2);          // (:310: consulted only when keyframe 1 has no stereo)
    const float cos_stereo = cos_stereo2 < cos_stereo1 ? cos_stereo2 : cos_stereo1;       // std::min(a, b): b < a ? b : a
    if (cos_rays < cos_stereo && cos_rays > 0 && (stereo1 || stereo2 || (double)cos_rays < 0.9998)) {
        // :320-338
        float A[4][4];
        for (int c = 0; c < 4; ++c) {
            const float r10 = c < 3 ? k1.Rcw[c] : k1.tcw[0], r11 = c < 3 ? k1.Rcw[3 + c] : k1.tcw[1], r12 = c < 3 ? k1.Rcw[6 + c] : k1.tcw[2];
            const float r20 = c < 3 ? k2.Rcw[c] : k2.tcw[0], r21 = c < 3 ? k2.Rcw[3 + c] : k2.tcw[1], r22 = c < 3 ? k2.Rcw[6 + c] : k2.tcw[2];
            A[0][c] = r12 * xn1[0] - r10;
            A[1][c] = r12 * xn1[1] - r11;
            A[2][c] = r22 * xn2[0] - r20;
            A[3][c] = r22 * xn2[1] - r21;
        }
        float e[4];
        tr_null_vector(A, e);
        if (e[3] == 0) { o.status = SIVO_TRI_W_ZERO; return; }
        const float inv = (float)(1.0 / (double)e[3]);
        for (int i = 0; i < 3; ++i) wP[i] = e[i] * inv;
    } else if (stereo1 && cos_stereo1 < cos_stereo2) {
        tr_unproject(k1, m.x1, m.y1, m.depth1, wP);
    } else if (stereo2 && cos_stereo2 < cos_stereo1) {
        tr_unproject(k2, m.x2, m.y2, m.depth2, wP);
    } else {
        return;
    }
    for (int i = 0; i < 3; ++i) o.wP[i] = wP[i];
    // :351-362
    const float z1 = (float)(tr_dot3(k1.Rcw + 6, wP) + (double)k1.tcw[2]);
    if (z1 <= 0) { o.status = SIVO_TRI_Z1; return; }
    const float z2 = (float)(tr_dot3(k2.Rcw + 6, wP) + (double)k2.tcw[2]);
    if (z2 <= 0) { o.status = SIVO_TRI_Z2; return; }
    // :364-425
    if (tr_reproj_fails(k1, wP, z1, stereo1, m.x1, m.y1, m.r1, k1.level_sigma2[m.octave1], k1.mbf)) { o.status = SIVO_TRI_REPROJ1; return; }
    if (tr_reproj_fails(k2, wP, z2, stereo2, m.x2, m.y2, m.r2, k2.level_sigma2[m.octave2], k1.mbf)) { o.status = SIVO_TRI_REPROJ2; return; }
    // :427-446
    const float n1[3] = {wP[0] - k1.Ow[0], wP[1] - k1.Ow[1], wP[2] - k1.Ow[2]};
    const float n2[3] = {wP[0] - k2.Ow[0], wP[1] - k2.Ow[1], wP[2] - k2.Ow[2]};
    const float dist1 = (float)sqrt(tr_dot3(n1, n1)), dist2 = (float)sqrt(tr_dot3(n2, n2));
    if (dist1 == 0 || dist2 == 0) { o.status = SIVO_TRI_ZERO_DIST; return; }
    const float ratio_dist = dist2 / dist1;
    const float ratio_octave = k1.scale_factors[m.octave1] / k2.scale_factors[m.octave2];
    if (ratio_dist * ratio_factor < ratio_octave || ratio_dist > ratio_octave * ratio_factor) { o.status = SIVO_TRI_SCALE; return; }
    // :449-452: CheckSemantics(keyframe 1, idx1, wP, true) (:474-545), CheckSemantics(keyframe 2, idx2, wP, false) = the bare class
    int cls = 255;
    if (m.depth1 > 0 && m.class1 <= 8 && m.confidence1 >= th_conf) {
        const double mi = gate_mutual_information(Sx, (double)k1.fx, (double)k1.fy, (double)k1.mb, (double)wP[0], (double)wP[1], (double)wP[2],
                                                  (double)k1.level_sigma2[m.octave1]);
        const double reduction = mi - m.entropy1;
        cls = reduction < th_ent ? 255 : (int)m.class1;
    }
    o.cls = (uint8_t)cls;
    o.status = (cls == (int)m.class2 && cls != 255) ? SIVO_TRI_ACCEPTED : SIVO_TRI_SEMANTICS;
}

// (sign and payload of a NaN depend on the machine that produced it: every NaN is stored as the quiet NaN 0x7FC00000)
SIVO_HD uint32_t tr_float_bits(float v) {
    union { float f; uint32_t u; } b;
    b.f = v;
    return v != v ? 0x7FC00000u : b.u;
}

}  // namespace sivo
