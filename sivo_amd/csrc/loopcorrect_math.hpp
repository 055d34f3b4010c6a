// loopcorrect_math.hpp — the per-item bodies of the two map corrections of the loop closer: LoopClosing::CorrectLoop's pose propagation
// and point correction (reference src/orbslam/LoopClosing.cc:436-526) and the map update behind the global bundle adjustment
// (LoopClosing.cc:694-753); shared by the kernels (loopcorrect.hip) and, compiled by g++, by the host programs of the tests.
//   * g2o::Sim3 in double with Eigen's operation order — the same operations as sim3_common.hpp, restated here because that header is
//     device-only; Quaterniond(R) is the trace-branch construction and is not normalised, toRotationMatrix is Eigen's.
//   * cv::Mat algebra in CV_32F under the rules of api/compat/cv_min.hpp: a product with no transposed operand and an inner dimension
//     of 2..4 is gemm's small-matrix path — each dot product accumulated left to right in float, then (float)(t * alpha + c * beta) in
//     double.  KeyFrame::SetPose (KeyFrame.cc:119-126) materialises Rwc = Rcw.t() before `-Rwc * tcw`, so that product has no
//     transposed operand either: the small path with alpha = -1.
//   * MapPoint::UpdateNormalAndDepth is the arithmetic of mp_normal_depth (mappoint_math.hpp) with the camera centres gathered through
//     the observation list instead of read from a packed array.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/sivo_hip.h"

#ifndef SIVO_HD
#ifdef __HIPCC__
#define SIVO_HD __host__ __device__ inline
#else
#define SIVO_HD inline
#endif
#endif

namespace sivo {

struct LcSim3 { double q[4], t[3], s; };

// Eigen's Quaternion * Vector3 (_transformVector): uv = q.vec x v; uv += uv; v + w uv + q.vec x uv
SIVO_HD void lc_quat_rotate(const double *q, const double *v, double *o) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    double u0 = y * v[2] - z * v[1], u1 = z * v[0] - x * v[2], u2 = x * v[1] - y * v[0];
    u0 = u0 + u0; u1 = u1 + u1; u2 = u2 + u2;
    o[0] = v[0] + w * u0 + (y * u2 - z * u1);
    o[1] = v[1] + w * u1 + (z * u0 - x * u2);
    o[2] = v[2] + w * u2 + (x * u1 - y * u0);
}

// s * (r * X) + t
SIVO_HD void lc_sim3_map(const LcSim3 &S, const double *X, double *Y) {
    double r[3];
    lc_quat_rotate(S.q, X, r);
    for (int i = 0; i < 3; ++i) Y[i] = S.s * r[i] + S.t[i];
}

// Sim3::operator*: r = ra rb, t = sa (ra tb) + ta, s = sa sb
SIVO_HD LcSim3 lc_sim3_mul(const LcSim3 &a, const LcSim3 &b) {
    LcSim3 o;
    const double ax = a.q[0], ay = a.q[1], az = a.q[2], aw = a.q[3], bx = b.q[0], by = b.q[1], bz = b.q[2], bw = b.q[3];
    o.q[0] = aw * bx + ax * bw + ay * bz - az * by;
    o.q[1] = aw * by + ay * bw + az * bx - ax * bz;
    o.q[2] = aw * bz + az * bw + ax * by - ay * bx;
    o.q[3] = aw * bw - ax * bx - ay * by - az * bz;
    double r[3];
    lc_quat_rotate(a.q, b.t, r);
    for (int i = 0; i < 3; ++i) o.t[i] = a.s * r[i] + a.t[i];
    o.s = a.s * b.s;
    return o;
}

// Sim3::inverse: (r^*, r^* ((-1/s) t), 1/s)
SIVO_HD LcSim3 lc_sim3_inv(const LcSim3 &a) {
    LcSim3 o;
    o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
    const double f = -1. / a.s;
    const double ft[3] = {f * a.t[0], f * a.t[1], f * a.t[2]};
    lc_quat_rotate(o.q, ft, o.t);
    o.s = 1. / a.s;
    return o;
}

SIVO_HD LcSim3 lc_sim3_load(const double *p) {
    LcSim3 S;
    for (int i = 0; i < 4; ++i) S.q[i] = p[i];
    for (int i = 0; i < 3; ++i) S.t[i] = p[4 + i];
    S.s = p[7];
    return S;
}

SIVO_HD double lc_canon(double v) {                     // a NaN leaves as the one quiet NaN, like the floats of the ABI
    if (v != v) {
        const uint64_t bits = 0x7FF8000000000000ull;
        double o;
        __builtin_memcpy(&o, &bits, 8);
        return o;
    }
    return v;
}
SIVO_HD float lc_canon(float v) {
    if (v != v) {
        const uint32_t bits = 0x7FC00000u;
        float o;
        __builtin_memcpy(&o, &bits, 4);
        return o;
    }
    return v;
}

SIVO_HD void lc_sim3_store(const LcSim3 &S, double *p) {
    for (int i = 0; i < 4; ++i) p[i] = lc_canon(S.q[i]);
    for (int i = 0; i < 3; ++i) p[4 + i] = lc_canon(S.t[i]);
    p[7] = lc_canon(S.s);
}

// g2o::Sim3(R, t, 1.0) of the top three rows of a float pose T (row-major, 4 columns): Quaterniond((double)R), not normalised
SIVO_HD LcSim3 lc_sim3_of_pose(const float *T) {
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)T[4 * r + c];
    LcSim3 o;
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) {
        double t = sqrt(tr + 1.0);
        o.q[3] = 0.5 * t;
        t = 0.5 / t;
        o.q[0] = (R[7] - R[5]) * t; o.q[1] = (R[2] - R[6]) * t; o.q[2] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
        o.q[i] = 0.5 * t;
        t = 0.5 / t;
        o.q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
        o.q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
        o.q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
    }
    for (int r = 0; r < 3; ++r) o.t[r] = (double)T[4 * r + 3];
    o.s = 1.0;
    return o;
}

// the tail of gemm's small-matrix path: (float)(t * alpha + c * beta), c * beta already formed in double (0.0 without a C operand)
SIVO_HD float lc_gemm_tail(float t, double alpha, double c) { return (float)((double)t * alpha + c); }

// D = A * B for two 4 x 4 CV_32F matrices (inner dimension 4: the small path); D must not alias A or B
SIVO_HD void lc_mul44(const float *A, const float *B, float *D) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float t = A[4 * i] * B[j];
            for (int k = 1; k < 4; ++k) t = t + A[4 * i + k] * B[4 * k + j];
            D[4 * i + j] = lc_gemm_tail(t, 1.0, 0.0);
        }
}

// y = R * x + c for the 3 x 3 block and a column of 4 x 4 poses (inner dimension 3, a C operand with beta = 1): Rx = the pose whose
// rotation block multiplies, cx = the pose whose fourth column is added
SIVO_HD void lc_rot_add(const float *Rx, const float *x, const float *cx, float *y) {
    for (int i = 0; i < 3; ++i) {
        float t = Rx[4 * i] * x[0];
        t = t + Rx[4 * i + 1] * x[1];
        t = t + Rx[4 * i + 2] * x[2];
        y[i] = lc_gemm_tail(t, 1.0, (double)cx[4 * i + 3] * 1.0);
    }
}

// KeyFrame::SetPose (KeyFrame.cc:119-126): Rwc = Rcw.t() materialised, Ow = -Rwc * tcw, Twc = [Rwc Ow; 0 0 0 1]
SIVO_HD void lc_pose_inverse(const float *Tcw, float *Twc) {
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) Twc[4 * i + k] = Tcw[4 * k + i];
        float t = Twc[4 * i] * Tcw[3];
        t = t + Twc[4 * i + 1] * Tcw[7];
        t = t + Twc[4 * i + 2] * Tcw[11];
        Twc[4 * i + 3] = lc_gemm_tail(t, -1.0, 0.0);
    }
    Twc[12] = 0.0f; Twc[13] = 0.0f; Twc[14] = 0.0f; Twc[15] = 1.0f;
}

// Converter::toCvSE3(toRotationMatrix(q), t * (1. / s)) (LoopClosing.cc:513-520): both narrowed to float
SIVO_HD void lc_pose_of_sim3(const LcSim3 &S, float *T) {
    const double x = S.q[0], y = S.q[1], z = S.q[2], w = S.q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                 tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double M[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
    const double f = 1. / S.s;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)M[3 * r + c];
        T[4 * r + 3] = (float)(S.t[r] * f);
    }
    T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

// ---- sivo_loop_correct ---------------------------------------------------------------------------------------------------------------
// Keyframe i of the corrected set (LoopClosing.cc:453-471, :482, :513-522): its two Sim3, the inverse of the corrected one for the points,
// the new pose and camera centre.  non / cor / cor_inv: 8 doubles each; tiw_out 16 floats; ow_out 3 floats.
SIVO_HD void lc_keyframe(const SivoLoopCorrect &a, int i, double *non, double *cor, double *cor_inv, float *tiw_out, float *ow_out) {
    const float *Tiw = a.tiw + 16 * (int64_t)i;
    const LcSim3 Siw = lc_sim3_of_pose(Tiw);
    const LcSim3 Scw = lc_sim3_load(a.scw);
    LcSim3 C;
    if (i != a.cur) {
        float Tic[16];
        lc_mul44(Tiw, a.twc_cur, Tic);
        C = lc_sim3_mul(lc_sim3_of_pose(Tic), Scw);
    } else {
        C = Scw;
    }
    lc_sim3_store(Siw, non);
    lc_sim3_store(C, cor);
    const LcSim3 Ci = lc_sim3_inv(C);
    for (int k = 0; k < 4; ++k) cor_inv[k] = Ci.q[k];
    for (int k = 0; k < 3; ++k) cor_inv[4 + k] = Ci.t[k];
    cor_inv[7] = Ci.s;
    float T[16], Twc[16];
    lc_pose_of_sim3(C, T);
    lc_pose_inverse(T, Twc);
    for (int k = 0; k < 16; ++k) tiw_out[k] = lc_canon(T[k]);
    for (int k = 0; k < 3; ++k) ow_out[k] = lc_canon(Twc[4 * k + 3]);
}

// The camera centre keyframe k has while keyframe `owner` walks its points (:508 before :522): the new one for the corrected keyframes
// the walk has left behind, the caller's for all others
SIVO_HD const float *lc_centre(const SivoLoopCorrect &a, const float *ow_new, int32_t owner, int32_t k) {
    return k < a.n_kf && k < owner ? ow_new + 3 * (int64_t)k : a.ow + 3 * (int64_t)k;
}

// Point p moved by keyframe `owner` (:498-508).  non / cor_inv: the arrays lc_keyframe wrote, ow_new its camera centres (NaNs made
// canonical, which no comparison or sum tells apart).  pos_out[3]; geom[5] = max, min, normal[3], written when the point has
// observations.  Returns the flags.
SIVO_HD uint8_t lc_point(const SivoLoopCorrect &a, const double *non, const double *cor_inv, const float *ow_new, int32_t owner, int32_t p,
                         float *pos_out, float *geom) {
    const float *P = a.pos + 3 * (int64_t)p;
    const double X[3] = {(double)P[0], (double)P[1], (double)P[2]};
    double Y[3], Z[3];
    lc_sim3_map(lc_sim3_load(non + 8 * (int64_t)owner), X, Y);
    lc_sim3_map(lc_sim3_load(cor_inv + 8 * (int64_t)owner), Y, Z);
    const float pos[3] = {(float)Z[0], (float)Z[1], (float)Z[2]};
    for (int i = 0; i < 3; ++i) pos_out[i] = lc_canon(pos[i]);
    const int64_t o0 = a.obs_off[p], M = a.obs_off[p + 1] - o0;
    if (M == 0) return SIVO_MP_NO_OBSERVATION;                          // (MapPoint.cc:385-387)
    float normal[3] = {0.0f, 0.0f, 0.0f};
    for (int64_t j = 0; j < M; ++j) {                                   // mp_normal_depth, the centres gathered
        const float *ow = lc_centre(a, ow_new, owner, a.obs_kf[o0 + j]);
        const float d[3] = {pos[0] - ow[0], pos[1] - ow[1], pos[2] - ow[2]};
        double s = 0.0;
        s += (double)d[0] * (double)d[0]; s += (double)d[1] * (double)d[1]; s += (double)d[2] * (double)d[2];
        const float f = (float)(1.0 / sqrt(s));
        normal[0] = normal[0] + d[0] * f; normal[1] = normal[1] + d[1] * f; normal[2] = normal[2] + d[2] * f;
    }
    const float *rw = lc_centre(a, ow_new, owner, a.ref_kf[p]);
    const float pc[3] = {pos[0] - rw[0], pos[1] - rw[1], pos[2] - rw[2]};
    double s = 0.0;
    s += (double)pc[0] * (double)pc[0]; s += (double)pc[1] * (double)pc[1]; s += (double)pc[2] * (double)pc[2];
    const float dist = (float)sqrt(s);
    const float mx = dist * a.level_scale[p];
    const float fn = (float)(1.0 / (double)M);
    geom[0] = lc_canon(mx);
    geom[1] = lc_canon(mx / a.last_scale[p]);
    geom[2] = lc_canon(normal[0] * fn); geom[3] = lc_canon(normal[1] * fn); geom[4] = lc_canon(normal[2] * fn);
    return 0;
}

// ---- sivo_gba_propagate --------------------------------------------------------------------------------------------------------------
// What the walk of :695-718 leaves in keyframe k.  parent[k]: the keyframe that lists k as a child, -1 for none; kf_flags[k]: LC_KF_ORIGIN,
// and LC_KF_REACHED where k's chain of parents ends in an origin — the walk comes by exactly those (the argument check visits every
// keyframe once anyway and leaves both).  mTcwGBA of a keyframe outside the BA depends on its parent's: the chain is recomputed downward
// from the nearest ancestor that is inside the BA or an origin (whose mTcwGBA the walk does not write), each link found by walking up
// again — no storage per thread, no thread waits for another, every loop bounded by n_kf.
//   gba[16], twc[16]: mTcwGBA and GetPoseInverse() after the walk; in_gba_after; returns whether k was reached (mTcwBefGBA is then
//   tcw[k], else it stays tcw_bef[k]).
enum { LC_KF_ORIGIN = 1, LC_KF_REACHED = 2 };
SIVO_HD bool lc_tree_keyframe(const SivoGbaPropagate &a, const int32_t *parent, const uint8_t *kf_flags, int32_t k, float *gba, float *twc,
                              uint8_t *in_gba_after) {
    if (!(kf_flags[k] & LC_KF_REACHED)) {
        for (int i = 0; i < 16; ++i) gba[i] = a.tcw_gba[16 * (int64_t)k + i];
        lc_pose_inverse(a.tcw + 16 * (int64_t)k, twc);
        *in_gba_after = a.in_gba[k];
        return false;
    }
    int32_t depth = 0, anchor = k;                                      // links from k up to its anchor (an origin at the latest)
    while (depth < a.n_kf && !(a.in_gba[anchor] || (kf_flags[anchor] & LC_KF_ORIGIN))) { anchor = parent[anchor]; ++depth; }
    float G[16];
    for (int i = 0; i < 16; ++i) G[i] = a.tcw_gba[16 * (int64_t)anchor + i];
    for (int32_t link = depth - 1; link >= 0; --link) {                 // (:707-709) for the keyframe `link` links above k
        int32_t c = k;
        for (int32_t d = 0; d < link; ++d) c = parent[c];
        float Twc[16], Tchildc[16], N[16];
        lc_pose_inverse(a.tcw + 16 * (int64_t)parent[c], Twc);          // the parent's GetPoseInverse() before its SetPose
        lc_mul44(a.tcw + 16 * (int64_t)c, Twc, Tchildc);
        lc_mul44(Tchildc, G, N);
        for (int i = 0; i < 16; ++i) G[i] = N[i];
    }
    for (int i = 0; i < 16; ++i) gba[i] = G[i];
    lc_pose_inverse(G, twc);                                            // (:716)
    *in_gba_after = depth > 0 ? 1 : a.in_gba[k];                        // (:710; an origin outside the BA stays outside)
    return true;
}

// One map point of :723-753.  reached / twc / in_gba_after: what lc_tree_keyframe left per keyframe.
SIVO_HD uint8_t lc_gba_point(const SivoGbaPropagate &a, const uint8_t *reached, const float *twc, const uint8_t *in_gba_after, int32_t p,
                             float *pos_out) {
    if (a.point_bad[p]) return SIVO_GBA_POINT_BAD;
    if (a.point_in_gba[p]) {
        for (int i = 0; i < 3; ++i) pos_out[i] = lc_canon(a.pos_gba[3 * (int64_t)p + i]);
        return SIVO_GBA_POINT_FROM_BA;
    }
    const int32_t r = a.ref_kf[p];
    if (!in_gba_after[r]) return SIVO_GBA_POINT_REF_OUTSIDE;
    const float *bef = (reached[r] ? a.tcw : a.tcw_bef) + 16 * (int64_t)r;          // mTcwBefGBA after the walk (:715)
    float Xc[3], Y[3];
    lc_rot_add(bef, a.pos + 3 * (int64_t)p, bef, Xc);
    lc_rot_add(twc + 16 * (int64_t)r, Xc, twc + 16 * (int64_t)r, Y);
    for (int i = 0; i < 3; ++i) pos_out[i] = lc_canon(Y[i]);
    return SIVO_GBA_POINT_CARRIED;
}

// ---- argument checks, host only: the text of what is wrong, or nullptr ---------------------------------------------------------------
inline const char *lc_check_csr(const int64_t *off, int64_t n, const char *null_text, const char *start_text, const char *order_text) {
    if (!off) return null_text;
    if (off[0] != 0) return start_text;
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return order_text;
    if (off[n] > ((int64_t)1 << 28)) return "more than 2^28 entries";
    return nullptr;
}

inline const char *lc_check_loop_correct(const SivoLoopCorrect *a) {
    if (!a) return "null problem";
    if (a->n_kf < 0 || a->n_all < 0 || a->n_points < 0) return "negative count";
    if (a->n_kf < 1) return "n_kf must be at least 1";
    if (a->n_all < a->n_kf) return "n_all is smaller than n_kf";
    if (a->n_all > (1 << 24) || a->n_points > (1 << 24)) return "more than 2^24 keyframes or points";
    if (a->cur < 0 || a->cur >= a->n_kf) return "cur outside 0 .. n_kf - 1";
    if (!a->tiw || !a->twc_cur || !a->scw || !a->ow) return "null keyframe array";
    if (!a->noncorrected_siw || !a->corrected_siw || !a->tiw_out || !a->ow_out) return "null keyframe output";
    if (!(a->scw[7] > 0.0)) return "scw scale is not positive";
    if (const char *e = lc_check_csr(a->slot_off, a->n_kf, "null slot_off", "slot_off does not start at 0", "slot_off decreases")) return e;
    const int64_t ns = a->slot_off[a->n_kf];
    if (ns && !a->slot_point) return "null slot_point";
    for (int64_t i = 0; i < ns; ++i)
        if (a->slot_point[i] < -1 || a->slot_point[i] >= a->n_points) return "slot_point outside -1 .. n_points - 1";
    if (a->n_points == 0) return nullptr;
    if (!a->pos || !a->skip || !a->ref_kf || !a->level_scale || !a->last_scale) return "null point array";
    if (!a->corrected_by || !a->pos_out || !a->normal || !a->max_dist || !a->min_dist || !a->flags) return "null point output";
    if (const char *e = lc_check_csr(a->obs_off, a->n_points, "null obs_off", "obs_off does not start at 0", "obs_off decreases")) return e;
    const int64_t no = a->obs_off[a->n_points];
    if (no && !a->obs_kf) return "null obs_kf";
    for (int64_t o = 0; o < no; ++o)
        if (a->obs_kf[o] < 0 || a->obs_kf[o] >= a->n_all) return "obs_kf outside 0 .. n_all - 1";
    for (int32_t p = 0; p < a->n_points; ++p)
        if (a->ref_kf[p] < -1 || a->ref_kf[p] >= a->n_all) return "ref_kf outside -1 .. n_all - 1";
    for (int64_t i = 0; i < ns; ++i) {
        const int32_t p = a->slot_point[i];
        if (p >= 0 && !a->skip[p] && a->ref_kf[p] < 0) return "a point that would be moved has no reference keyframe";
    }
    return nullptr;
}

// parent (n_kf) and kf_flags (n_kf: LC_KF_ORIGIN | LC_KF_REACHED) are filled on the way: the kernels walk them, so nothing that could make
// that walk endless passes
inline const char *lc_check_gba_propagate(const SivoGbaPropagate *a, int32_t *parent, uint8_t *kf_flags) {
    if (!a) return "null problem";
    if (a->n_kf < 0 || a->n_origins < 0 || a->n_points < 0) return "negative count";
    if (a->n_kf > (1 << 24) || a->n_points > (1 << 24)) return "more than 2^24 keyframes or points";
    if (a->n_origins && !a->origin) return "null origin";
    for (int32_t i = 0; i < a->n_origins; ++i)
        if (a->origin[i] < 0 || a->origin[i] >= a->n_kf) return "origin outside 0 .. n_kf - 1";
    if (a->n_kf) {
        if (!a->tcw || !a->tcw_gba || !a->in_gba || !a->tcw_bef) return "null keyframe array";
        if (!a->tcw_out || !a->ow_out || !a->kf_reached) return "null keyframe output";
        if (const char *e = lc_check_csr(a->child_off, a->n_kf, "null child_off", "child_off does not start at 0", "child_off decreases")) return e;
        const int64_t nc = a->child_off[a->n_kf];
        if (nc && !a->child_kf) return "null child_kf";
        for (int64_t i = 0; i < nc; ++i)
            if (a->child_kf[i] < 0 || a->child_kf[i] >= a->n_kf) return "child_kf outside 0 .. n_kf - 1";
        for (int32_t k = 0; k < a->n_kf; ++k) { parent[k] = -1; kf_flags[k] = 0; }
        for (int32_t k = 0; k < a->n_kf; ++k)
            for (int64_t i = a->child_off[k]; i < a->child_off[k + 1]; ++i) {
                if (parent[a->child_kf[i]] >= 0) return "a keyframe is listed as a child more than once";
                parent[a->child_kf[i]] = k;
            }
        for (int32_t i = 0; i < a->n_origins; ++i) {
            if (parent[a->origin[i]] >= 0) return "an origin is somebody's child";
            if (kf_flags[a->origin[i]]) return "an origin is listed more than once";
            kf_flags[a->origin[i]] = 1;
        }
        // one parent each: a cycle is a chain of parents that never ends.  kf_flags doubles as the colour while the chains are
        // walked: 2 = on the chain being walked, 4 = known to end
        for (int32_t k = 0; k < a->n_kf; ++k) {
            int32_t n = k;
            while (n >= 0 && !(kf_flags[n] & 6)) { kf_flags[n] |= 2; n = parent[n]; }
            const bool cycle = n >= 0 && (kf_flags[n] & 2) && !(kf_flags[n] & 4);
            if (cycle) return "the children form a cycle";
            for (n = k; n >= 0 && (kf_flags[n] & 2) && !(kf_flags[n] & 4); n = parent[n]) kf_flags[n] = (uint8_t)((kf_flags[n] & 1) | 4);
        }
        for (int32_t k = 0; k < a->n_kf; ++k) kf_flags[k] &= 1;
        // reached: the chain of parents ends in an origin.  Bit 8 = known; every keyframe is settled once
        for (int32_t k = 0; k < a->n_kf; ++k) {
            int32_t n = k;
            while (!(kf_flags[n] & 8) && parent[n] >= 0) n = parent[n];
            const uint8_t r = (kf_flags[n] & 8) ? (uint8_t)(kf_flags[n] & LC_KF_REACHED) : (uint8_t)((kf_flags[n] & LC_KF_ORIGIN) ? LC_KF_REACHED : 0);
            for (int32_t m = k; !(kf_flags[m] & 8); m = parent[m]) {
                kf_flags[m] |= (uint8_t)(8 | r);
                if (m == n) break;
            }
        }
        for (int32_t k = 0; k < a->n_kf; ++k) kf_flags[k] &= (LC_KF_ORIGIN | LC_KF_REACHED);
    }
    if (a->n_points == 0) return nullptr;
    if (!a->pos || !a->pos_gba || !a->point_in_gba || !a->point_bad || !a->ref_kf) return "null point array";
    if (!a->pos_out || !a->point_status) return "null point output";
    for (int32_t p = 0; p < a->n_points; ++p) {
        if (a->ref_kf[p] < -1 || a->ref_kf[p] >= a->n_kf) return "ref_kf outside -1 .. n_kf - 1";
        if (!a->point_bad[p] && !a->point_in_gba[p] && a->ref_kf[p] < 0) return "a point that would be carried has no reference keyframe";
    }
    return nullptr;
}

}  // namespace sivo
