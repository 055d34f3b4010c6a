// The reference signatures of SIVO::Optimizer over the SLAM object graph (reference include/orbslam/Optimizer.h:46-60):
//     int  Optimizer::PoseOptimization(Frame *pFrame)                                  Optimizer.cc:273-491
//     void Optimizer::LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *)    Optimizer.cc:493-926
//     void Optimizer::BundleAdjustment(vpKF, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust)      Optimizer.cc:49-271
//     void Optimizer::GlobalBundleAdjustment(Map *, nIterations, pbStopFlag, nLoopKF, bRobust)     Optimizer.cc:37-47
// as header-only templates (free functions, and the static members of class Optimizer that forward to them): the graph walk the reference does in front of g2o (which observations become edges, mono
// or stereo by mvRight, information = mvInvLevelSigma2[octave], which keyframes are fixed) fills SivoEdge arrays, the
// array-level Optimizer entry points (GPU: Levenberg-Marquardt + Schur, chi2 schedules, marginal covariance) do what
// g2o + CHOLMOD do, and the results are written back the way the reference does (SetPose, mvbOutlier, SetCovariance,
// EraseMapPointMatch / EraseObservation under the map mutex, SetWorldPos + UpdateNormalAndDepth).
//
// Frame / KeyFrame / MapPoint / Map are template parameters (SLAM data model, outside this library — SURVEY.md 8): any
// types exposing the members used below under the reference's names compile, the reference's own classes included.
// tests/cpp/test_api.cpp instantiates both with minimal stand-ins.
#ifndef OPTIMIZER_ADAPTER_H
#define OPTIMIZER_ADAPTER_H

#include <cmath>
#include <cstring>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "LocalMapAdapter.h"
#include "Optimizer.h"

#ifdef SIVO_HAVE_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "../compat/cv_min.hpp"
#endif
#ifdef SIVO_HAVE_EIGEN
#include <Eigen/Core>      // Frame / KeyFrame::SetCovariance(Eigen::MatrixXd) (reference Frame.cc:254-260)
#endif

namespace SIVO {
namespace optimizer_detail {

// Converter::toSE3Quat (reference src/orbslam/Converter.cc:33-42) turns the float pose into an Eigen quaternion (unit
// norm) + translation, and g2o works with the rotation matrix of THAT quaternion: the float matrix is re-orthogonalised
// on the way in.  Same here: matrix -> quaternion (the trace-branch construction Eigen uses) -> normalise -> matrix.
inline void se3_from_cv(const cv::Mat &Tcw, double pose[12]) {
    double R[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r][c] = Tcw.at<float>(r, c);
    double q[4];     // x y z w
    const double t = R[0][0] + R[1][1] + R[2][2];
    if (t > 0.0) {
        double s = std::sqrt(t + 1.0);
        q[3] = 0.5 * s;
        s = 0.5 / s;
        q[0] = (R[2][1] - R[1][2]) * s; q[1] = (R[0][2] - R[2][0]) * s; q[2] = (R[1][0] - R[0][1]) * s;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (R[2][2] > R[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
        q[i] = 0.5 * s;
        s = 0.5 / s;
        q[3] = (R[k][j] - R[j][k]) * s; q[j] = (R[j][i] + R[i][j]) * s; q[k] = (R[k][i] + R[i][k]) * s;
    }
    const double nrm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (double &v : q) v /= nrm;
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                 tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double M[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
    for (int i = 0; i < 9; ++i) pose[i] = M[i];
    for (int r = 0; r < 3; ++r) pose[9 + r] = Tcw.at<float>(r, 3);
}

// Converter::toCvMat(g2o::SE3Quat) (Converter.cc:44-48): 4 x 4 CV_32F
inline cv::Mat cv_from_se3(const double pose[12]) {
    cv::Mat T = cv::Mat::zeros(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T.at<float>(r, c) = (float)pose[3 * r + c];
        T.at<float>(r, 3) = (float)pose[9 + r];
    }
    T.at<float>(3, 3) = 1.f;
    return T;
}

// one observation as the reference sets it up (Optimizer.cc:318-409 resp. 668-755)
template <class FrameLike>
SivoEdge observation(const FrameLike &F, size_t idx, int pose, int point) {
    SivoEdge e{};
    const cv::KeyPoint &kp = F.mvKeysSemantic[idx];
    e.pose = pose; e.point = point;
    e.obs[0] = kp.pt.x; e.obs[1] = kp.pt.y;
    e.stereo = F.mvRight[idx] < 0 ? 0 : 1;
    if (e.stereo) e.obs[2] = F.mvRight[idx];
    e.inv_sigma2 = F.mvInvLevelSigma2[kp.octave];
    return e;
}

template <class T>
void set_covariance(T *obj, const double cov[36]) {
#ifdef SIVO_HAVE_EIGEN
    Eigen::MatrixXd S(6, 6);
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) S(r, c) = cov[6 * r + c];
    obj->SetCovariance(S);
#else
    obj->SetCovariance(cov);      // 6 x 6 row-major
#endif
}

// `R * X + t` of two CV_32F cv::Mats (3 x 3 by 3 x 1): gemm's small-matrix path, each dot product summed left to right in float,
// then + t — the arithmetic ORBmatcher.h's matcher_detail::Pose::apply restates (pinned against the reference there)
inline void cv_rx_plus_t(const cv::Mat &R, const cv::Mat &t, const cv::Mat &X, double out[3]) {
    for (int r = 0; r < 3; ++r) {
        float s = R.at<float>(r, 0) * X.at<float>(0, 0);
        s = s + R.at<float>(r, 1) * X.at<float>(1, 0);
        s = s + R.at<float>(r, 2) * X.at<float>(2, 0);
        out[r] = (double)(s + t.at<float>(r, 0));
    }
}

// The correspondences of Optimizer::OptimizeSim3 (Optimizer.cc:1294-1383): pair i of vpMatches1 enters when vpMatches1[i] and
// pKF1's own map point i are both set and not bad and the match has an index in pKF2 (GetIndexInKeyFrame >= 0).  index[k] = i of
// the k-th pair.  Points in camera coordinates with the float rounding of `R * Xw + t`; keypoints from mvKeysSemantic,
// information mvInvLevelSigma2[octave].
template <class KeyFrameT, class MapPointT>
void gather_sim3(KeyFrameT *pKF1, KeyFrameT *pKF2, const std::vector<MapPointT *> &vpMatches1, std::vector<SivoSim3Match> &pairs,
                 std::vector<size_t> &index) {
    pairs.clear(); index.clear();
    const cv::Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation();
    const cv::Mat R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
    const auto vpMapPoints1 = pKF1->GetMapPointMatches();
    const int N = (int)vpMatches1.size();
    for (int i = 0; i < N; ++i) {
        if (!vpMatches1[i]) continue;
        MapPointT *pMP1 = vpMapPoints1[i];
        MapPointT *pMP2 = vpMatches1[i];
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (!pMP1 || pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
        SivoSim3Match m{};
        cv_rx_plus_t(R1w, t1w, pMP1->GetWorldPos(), m.x1c);
        cv_rx_plus_t(R2w, t2w, pMP2->GetWorldPos(), m.x2c);
        const cv::KeyPoint &kp1 = pKF1->mvKeysSemantic[i];
        m.obs1[0] = kp1.pt.x; m.obs1[1] = kp1.pt.y;
        m.inv_sigma2_1 = pKF1->mvInvLevelSigma2[kp1.octave];
        const cv::KeyPoint &kp2 = pKF2->mvKeysSemantic[i2];
        m.obs2[0] = kp2.pt.x; m.obs2[1] = kp2.pt.y;
        m.inv_sigma2_2 = pKF2->mvInvLevelSigma2[kp2.octave];
        pairs.push_back(m);
        index.push_back((size_t)i);
    }
}

// g2o::Sim3's rotation() is an Eigen quaternion; a stand-in may hand out a 3 x 3 matrix instead.  Read / write either as
// (x, y, z, w); a matrix goes through Eigen's Quaternion(const Matrix3 &) construction (the trace branch) and back.
template <class Q>
auto sim3_rot_get(const Q &q, double o[4], int) -> decltype((void)q.w()) {
    o[0] = q.x(); o[1] = q.y(); o[2] = q.z(); o[3] = q.w();
}
template <class M>
void sim3_rot_get(const M &R, double o[4], long) {
    const double t = R(0, 0) + R(1, 1) + R(2, 2);
    if (t > 0.0) {
        double s = std::sqrt(t + 1.0);
        o[3] = 0.5 * s;
        s = 0.5 / s;
        o[0] = (R(2, 1) - R(1, 2)) * s; o[1] = (R(0, 2) - R(2, 0)) * s; o[2] = (R(1, 0) - R(0, 1)) * s;
    } else {
        int i = 0;
        if (R(1, 1) > R(0, 0)) i = 1;
        if (R(2, 2) > R(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = std::sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0);
        o[i] = 0.5 * s;
        s = 0.5 / s;
        o[3] = (R(k, j) - R(j, k)) * s; o[j] = (R(j, i) + R(i, j)) * s; o[k] = (R(k, i) + R(i, k)) * s;
    }
}
template <class Q>
auto sim3_rot_set(Q &q, const double v[4], int) -> decltype((void)(q.w() = 0.0)) {
    q.x() = v[0]; q.y() = v[1]; q.z() = v[2]; q.w() = v[3];
}
template <class M>
void sim3_rot_set(M &R, const double v[4], long) {
    const double x = v[0], y = v[1], z = v[2], w = v[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                 tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R(0, 0) = 1 - (tyy + tzz); R(0, 1) = txy - twz;       R(0, 2) = txz + twy;
    R(1, 0) = txy + twz;       R(1, 1) = 1 - (txx + tzz); R(1, 2) = tyz - twx;
    R(2, 0) = txz - twy;       R(2, 1) = tyz + twx;       R(2, 2) = 1 - (txx + tyy);
}

// g2o::Sim3 on the host, for the measurements of OptimizeEssentialGraph: (x y z w, t, s) with the product and inverse in Eigen's
// operation order (the device's sim3_common.hpp restates the same)
struct HostSim3 { double q[4], t[3], s; };
inline void host_quat_rotate(const double q[4], const double v[3], double o[3]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    double u0 = y * v[2] - z * v[1], u1 = z * v[0] - x * v[2], u2 = x * v[1] - y * v[0];
    u0 = u0 + u0; u1 = u1 + u1; u2 = u2 + u2;
    o[0] = v[0] + w * u0 + (y * u2 - z * u1);
    o[1] = v[1] + w * u1 + (z * u0 - x * u2);
    o[2] = v[2] + w * u2 + (x * u1 - y * u0);
}
inline HostSim3 host_sim3_mul(const HostSim3 &a, const HostSim3 &b) {
    HostSim3 o;
    const double ax = a.q[0], ay = a.q[1], az = a.q[2], aw = a.q[3], bx = b.q[0], by = b.q[1], bz = b.q[2], bw = b.q[3];
    o.q[0] = aw * bx + ax * bw + ay * bz - az * by;
    o.q[1] = aw * by + ay * bw + az * bx - ax * bz;
    o.q[2] = aw * bz + az * bw + ax * by - ay * bx;
    o.q[3] = aw * bw - ax * bx - ay * by - az * bz;
    double r[3];
    host_quat_rotate(a.q, b.t, r);
    for (int i = 0; i < 3; ++i) o.t[i] = a.s * r[i] + a.t[i];
    o.s = a.s * b.s;
    return o;
}
inline HostSim3 host_sim3_inv(const HostSim3 &a) {
    HostSim3 o;
    o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
    const double f = -1. / a.s;
    const double ft[3] = {f * a.t[0], f * a.t[1], f * a.t[2]};
    host_quat_rotate(o.q, ft, o.t);
    o.s = 1. / a.s;
    return o;
}
// g2o::Sim3(Rcw, tcw, 1.0) from a keyframe pose (Optimizer.cc:984-989): Quaterniond(R) of the float rotation, not normalised
template <class KeyFrameT>
HostSim3 host_sim3_of_pose(KeyFrameT *pKF) {
    const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation();
    double M[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) M[r][c] = R.at<float>(r, c);
    struct { const double (*m)[3]; double operator()(int r, int c) const { return m[r][c]; } } Rm{M};
    HostSim3 S;
    sim3_rot_get(Rm, S.q, 0);
    for (int r = 0; r < 3; ++r) S.t[r] = t.at<float>(r, 0);
    S.s = 1.0;
    return S;
}
template <class Sim3T>
HostSim3 host_sim3_of(const Sim3T &g) {
    HostSim3 S;
    sim3_rot_get(g.rotation(), S.q, 0);
    const auto t = g.translation();
    for (int i = 0; i < 3; ++i) S.t[i] = t[i];
    S.s = g.scale();
    return S;
}
inline void host_sim3_store(const HostSim3 &S, double o[8]) {
    for (int i = 0; i < 4; ++i) o[i] = S.q[i];
    for (int i = 0; i < 3; ++i) o[4 + i] = S.t[i];
    o[7] = S.s;
}
inline HostSim3 host_sim3_load(const double o[8]) {
    HostSim3 S;
    for (int i = 0; i < 4; ++i) S.q[i] = o[i];
    for (int i = 0; i < 3; ++i) S.t[i] = o[4 + i];
    S.s = o[7];
    return S;
}

// The graph of Optimizer::OptimizeEssentialGraph (Optimizer.cc:964-1175), in the reference's order.  siw[8 (maxKFid + 1)]: vScw —
// the vertex estimates (CorrectedSim3 if present, else Sim3(Rcw, tcw, 1)), identity where there is no vertex; fixed: pLoopKF;
// vertex: which ids have one.  Edges: first the LoopConnections (weight >= 100, or the (pCurKF, pLoopKF) pair; measurements from
// vScw), then per keyframe of GetAllKeyFrames() the spanning-tree edge, the loop edges to smaller ids and the covisibility edges
// (GetCovisiblesByWeight(100), smaller id, not parent / child / loop edge / bad / already a LoopConnections pair), their Swi / Sjw
// from NonCorrectedSim3 where present.  A bad keyframe in the list is skipped in the normal-edge walk, and an edge to a keyframe
// without a vertex is left out: the reference would hand g2o a null vertex there.
template <class MapT, class KeyFrameT, class KFPoseMapT, class ConnectionsT>
void gather_essential_graph(MapT *pMap, KeyFrameT *pLoopKF, KeyFrameT *pCurKF, const KFPoseMapT &NonCorrectedSim3,
                            const KFPoseMapT &CorrectedSim3, const ConnectionsT &LoopConnections, std::vector<double> &siw,
                            std::vector<uint8_t> &fixed, std::vector<uint8_t> &vertex, std::vector<SivoSim3Edge> &edges) {
    const auto vpKFs = pMap->GetAllKeyFrames();
    const size_t n = (size_t)pMap->GetMaxKFid() + 1;
    const double I[8] = {0, 0, 0, 1, 0, 0, 0, 1};
    siw.assign(8 * n, 0.0);
    for (size_t v = 0; v < n; ++v) std::memcpy(&siw[8 * v], I, sizeof I);
    fixed.assign(n, 0);
    vertex.assign(n, 0);
    edges.clear();
    for (KeyFrameT *pKF : vpKFs) {                                   // vertices (:964-1006)
        if (pKF->isBad()) continue;
        const size_t id = (size_t)pKF->mnId;
        if (id >= n) continue;
        const auto it = CorrectedSim3.find(pKF);
        const HostSim3 S = it != CorrectedSim3.end() ? host_sim3_of(it->second) : host_sim3_of_pose(pKF);
        host_sim3_store(S, &siw[8 * id]);
        vertex[id] = 1;
        if (pKF == pLoopKF) fixed[id] = 1;
    }
    auto has_vertex = [&](size_t id) { return id < n && vertex[id]; };
    auto add = [&](size_t i, size_t j, const HostSim3 &Sji) {
        if (!has_vertex(i) || !has_vertex(j)) return;
        SivoSim3Edge e{};
        e.i = (int32_t)i; e.j = (int32_t)j;
        host_sim3_store(Sji, e.meas);
        edges.push_back(e);
    };
    const int minFeat = 100;
    std::set<std::pair<unsigned long, unsigned long>> sInsertedEdges;
    for (const auto &conn : LoopConnections) {                      // loop edges (:1011-1049)
        KeyFrameT *pKF = conn.first;
        const unsigned long nIDi = pKF->mnId;
        const HostSim3 Swi = host_sim3_inv(nIDi < n ? host_sim3_load(&siw[8 * nIDi]) : host_sim3_load(I));
        for (KeyFrameT *pKFj : conn.second) {
            const unsigned long nIDj = pKFj->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(pKFj) < minFeat) continue;
            const HostSim3 Sjw = nIDj < n ? host_sim3_load(&siw[8 * nIDj]) : host_sim3_load(I);
            add(nIDi, nIDj, host_sim3_mul(Sjw, Swi));
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    auto s_w = [&](KeyFrameT *pK) {                                   // NonCorrectedSim3 if present, else vScw
        const auto it = NonCorrectedSim3.find(pK);
        if (it != NonCorrectedSim3.end()) return host_sim3_of(it->second);
        const size_t id = (size_t)pK->mnId;
        return id < n ? host_sim3_load(&siw[8 * id]) : host_sim3_load(I);
    };
    for (KeyFrameT *pKF : vpKFs) {                                   // normal edges (:1052-1175)
        if (pKF->isBad()) continue;
        const unsigned long nIDi = pKF->mnId;
        const HostSim3 Swi = host_sim3_inv(s_w(pKF));
        KeyFrameT *pParentKF = pKF->GetParent();
        if (pParentKF) add(nIDi, pParentKF->mnId, host_sim3_mul(s_w(pParentKF), Swi));
        const auto sLoopEdges = pKF->GetLoopEdges();
        for (KeyFrameT *pLKF : sLoopEdges)
            if (pLKF->mnId < pKF->mnId) add(nIDi, pLKF->mnId, host_sim3_mul(s_w(pLKF), Swi));
        const auto vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (KeyFrameT *pKFn : vpConnectedKFs) {
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    add(nIDi, pKFn->mnId, host_sim3_mul(s_w(pKFn), Swi));
                }
            }
        }
    }
}

// SetPose of the write-back (Optimizer.cc:1184-1203): Sim3 [sR t] -> SE3 [R t/s]: R = toRotationMatrix, eigt *= 1. / s, both to float
inline cv::Mat cv_pose_from_sim3(const double S[8]) {
    double R[9];
    {
        const double x = S[0], y = S[1], z = S[2], w = S[3];
        const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                     tyy = ty * y, tyz = tz * y, tzz = tz * z;
        const double M[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
        for (int i = 0; i < 9; ++i) R[i] = M[i];
    }
    const double f = 1. / S[7];
    cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T.at<float>(r, c) = (float)R[3 * r + c];
        T.at<float>(r, 3) = (float)(S[4 + r] * f);
    }
    return T;
}

}  // namespace optimizer_detail

// void Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale)
// (Optimizer.cc:928-1233) on the device: the graph gathered as the reference builds it, optimize(20) (sivo_essential_graph_optimize),
// then under pMap->mMutexMapUpdate the keyframe poses (SetPose([R | t/s])) and the map points (correctedSwr.map(Srw.map(P)),
// sivo_sim3_correct_points; SetWorldPos + UpdateNormalAndDepth).  Keyframes that are bad or have no vertex are skipped in the
// write-back (the reference would dereference a null vertex there); a point whose reference keyframe has no vertex keeps its position
// (the reference maps it through two identities).
template <class MapT, class KeyFrameT, class KFPoseMapT, class ConnectionsT>
void OptimizeEssentialGraph(MapT *pMap, KeyFrameT *pLoopKF, KeyFrameT *pCurKF, const KFPoseMapT &NonCorrectedSim3, const KFPoseMapT &CorrectedSim3,
                            const ConnectionsT &LoopConnections, const bool &bFixScale) {
    using namespace optimizer_detail;
    std::vector<double> siw;
    std::vector<uint8_t> fixed, vertex;
    std::vector<SivoSim3Edge> edges;
    gather_essential_graph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, siw, fixed, vertex, edges);
    const std::vector<double> vScw = siw;
    const int n = (int)fixed.size();
    int rc = sivo_essential_graph_optimize(siw.data(), fixed.data(), n, edges.data(), (int)edges.size(), bFixScale ? 1 : 0, 20, nullptr,
                                           nullptr, nullptr);
    if (rc != SIVO_OK) throw std::runtime_error(std::string("sivo_essential_graph_optimize: ") + sivo_last_error());
    const auto vpKFs = pMap->GetAllKeyFrames();
    const auto vpMPs = pMap->GetAllMapPoints();
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (KeyFrameT *pKFi : vpKFs) {
        const size_t id = (size_t)pKFi->mnId;
        if (pKFi->isBad() || id >= (size_t)n || !vertex[id]) continue;      // (no vertex: the reference dereferences null here)
        pKFi->SetPose(cv_pose_from_sim3(&siw[8 * id]));
    }
    std::vector<decltype(vpMPs.size())> which;
    std::vector<float> xyz;
    std::vector<int32_t> ref;
    for (size_t i = 0; i < vpMPs.size(); ++i) {
        auto *pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        long nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = (long)pMP->mnCorrectedReference;
        else nIDr = (long)pMP->GetReferenceKeyFrame()->mnId;
        const cv::Mat P = pMP->GetWorldPos();
        for (int r = 0; r < 3; ++r) xyz.push_back(P.at<float>(r, 0));
        ref.push_back(nIDr >= 0 && nIDr < n && vertex[(size_t)nIDr] ? (int32_t)nIDr : -1);
        which.push_back(i);
    }
    std::vector<float> out(xyz.size());
    rc = sivo_sim3_correct_points(xyz.data(), ref.data(), (int)ref.size(), vScw.data(), siw.data(), n, out.data());
    if (rc != SIVO_OK) throw std::runtime_error(std::string("sivo_sim3_correct_points: ") + sivo_last_error());
    for (size_t k = 0; k < which.size(); ++k) {
        auto *pMP = vpMPs[which[k]];
        cv::Mat X(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) X.at<float>(r, 0) = out[3 * k + r];
        pMP->SetWorldPos(X);
        pMP->UpdateNormalAndDepth();
    }
}

// int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (Optimizer.cc:1236-1449) on the device: the pairs
// gathered as the reference builds its graph, the whole optimisation (sivo_sim3_optimize), vpMatches1[i] nulled for every
// outlier pair, g2oS12 written back through Sim3T's (rotation, translation, scale) constructor unless the reference returns
// before that (fewer than 10 pairs survive the first test: 0, g2oS12 untouched).  Returns the inlier count.
template <class KeyFrameT, class MapPointT, class Sim3T>
int OptimizeSim3(KeyFrameT *pKF1, KeyFrameT *pKF2, std::vector<MapPointT *> &vpMatches1, Sim3T &g2oS12, const float th2,
                 const bool bFixScale) {
    using namespace optimizer_detail;
    std::vector<SivoSim3Match> pairs;
    std::vector<size_t> index;
    gather_sim3(pKF1, pKF2, vpMatches1, pairs, index);
    const cv::Mat &K1 = pKF1->mK, &K2 = pKF2->mK;
    const double k1[4] = {K1.at<float>(0, 0), K1.at<float>(1, 1), K1.at<float>(0, 2), K1.at<float>(1, 2)};
    const double k2[4] = {K2.at<float>(0, 0), K2.at<float>(1, 1), K2.at<float>(0, 2), K2.at<float>(1, 2)};
    double s12[8], s_in[8];
    sim3_rot_get(g2oS12.rotation(), s12, 0);
    const auto t0 = g2oS12.translation();
    for (int i = 0; i < 3; ++i) s12[4 + i] = t0[i];
    s12[7] = g2oS12.scale();
    std::memcpy(s_in, s12, sizeof s12);
    std::vector<uint8_t> outlier(pairs.size());
    int nIn = 0;
    const int rc = sivo_sim3_optimize(s12, k1, k2, pairs.data(), (int)pairs.size(), th2, bFixScale ? 1 : 0, outlier.data(), &nIn,
                                      nullptr, nullptr, nullptr, nullptr);
    if (rc != SIVO_OK) throw std::runtime_error(std::string("sivo_sim3_optimize: ") + sivo_last_error());
    for (size_t k = 0; k < pairs.size(); ++k)
        if (outlier[k]) vpMatches1[index[k]] = nullptr;
    if (nIn > 0 || std::memcmp(s12, s_in, sizeof s12) != 0) {
        typename std::decay<decltype(g2oS12.rotation())>::type r = g2oS12.rotation();
        typename std::decay<decltype(g2oS12.translation())>::type t = g2oS12.translation();
        sim3_rot_set(r, s12, 0);
        for (int i = 0; i < 3; ++i) t[i] = s12[4 + i];
        g2oS12 = Sim3T(r, t, s12[7]);
    }
    return nIn;
}

// int Optimizer::PoseOptimization(Frame *pFrame)
template <class FrameT>
int PoseOptimization(FrameT *pFrame) {
    using namespace optimizer_detail;
    const int N = pFrame->numSemanticKeys;
    std::vector<SivoEdge> edges;
    std::vector<size_t> index;
    std::vector<double> points;
    edges.reserve((size_t)N); index.reserve((size_t)N); points.reserve(3 * (size_t)N);
    {
        // (the reference holds MapPoint::mGlobalMutex here, :312; the stand-in types decide what that means)
        for (int i = 0; i < N; ++i) {
            auto *pMP = pFrame->mvpMapPoints[i];
            if (!pMP) continue;
            pFrame->mvbOutlier[i] = false;
            const cv::Mat Xw = pMP->GetWorldPos();
            edges.push_back(observation(*pFrame, (size_t)i, 0, (int)index.size()));
            index.push_back((size_t)i);
            for (int r = 0; r < 3; ++r) points.push_back(Xw.at<float>(r, 0));
        }
    }
    const int nInitialCorrespondences = (int)edges.size();
    if (nInitialCorrespondences < 3) return 0;                                   // :409-411
    double pose[12], cov[36];
    se3_from_cv(pFrame->mTcw, pose);
    const double intr[5] = {pFrame->fx, pFrame->fy, pFrame->cx, pFrame->cy, pFrame->mbf};
    std::vector<uint8_t> outlier;
    bool covOk = false;
    const int inliers = Optimizer::PoseOptimization(pose, points, edges, intr, outlier, cov, &covOk);
    for (size_t e = 0; e < edges.size(); ++e) pFrame->mvbOutlier[index[e]] = outlier[e] != 0;
    pFrame->SetPose(cv_from_se3(pose));                                          // :470-475
    if (covOk) set_covariance(pFrame, cov);                                      // :477-485
    return inliers;
}

namespace optimizer_detail {

// What Optimizer::LocalBundleAdjustment hands to the optimiser (Optimizer.cc:496-755): the window's keyframes and points in the
// reference's order, the vertices as arrays (local keyframes first, keyframe 0 of the map held fixed, then the fixed ones), one SivoEdge
// per observation and the objects behind each edge.
template <class KeyFrameT, class MapPointT>
struct LocalBAProblem {
    std::vector<KeyFrameT *> localKFs;          // lLocalKeyFrames
    std::vector<MapPointT *> localPoints;       // lLocalMapPoints
    std::map<KeyFrameT *, int> poseIndex;
    std::vector<double> poses;
    std::vector<uint8_t> fixedPose;
    std::vector<double> points;
    std::vector<SivoEdge> edges;
    std::vector<KeyFrameT *> edgeKF;
    std::vector<MapPointT *> edgeMP;

    void add_pose(KeyFrameT *k, bool fixed) {                                    // (:585-622)
        double p[12];
        se3_from_cv(k->GetPose(), p);
        poseIndex[k] = (int)fixedPose.size();
        poses.insert(poses.end(), p, p + 12);
        fixedPose.push_back(fixed ? 1 : 0);
    }
    void add_point(MapPointT *pMP) {                                             // (:655-656)
        const cv::Mat Xw = pMP->GetWorldPos();
        for (int r = 0; r < 3; ++r) points.push_back(Xw.at<float>(r, 0));
    }
    void add_edge(KeyFrameT *pKFi, MapPointT *pMP, size_t idx, int pose, int point) {       // (:668-755)
        edges.push_back(observation(*pKFi, idx, pose, point));
        edgeKF.push_back(pKFi); edgeMP.push_back(pMP);
    }
};

template <class KeyFrameT>
struct MapPointOf {
    typedef typename std::remove_pointer<typename decltype(std::declval<KeyFrameT *>()->GetMapPointMatches())::value_type>::type type;
};

// The walk over the object graph (Optimizer.cc:496-559, :585-622, :651-670)
template <class KeyFrameT>
LocalBAProblem<KeyFrameT, typename MapPointOf<KeyFrameT>::type> gather_local_ba(KeyFrameT *pKF) {
    typedef typename MapPointOf<KeyFrameT>::type MapPointT;
    LocalBAProblem<KeyFrameT, MapPointT> P;
    // local keyframes: the current one and its covisible neighbours (:496-512)
    std::list<KeyFrameT *> lLocalKeyFrames;
    lLocalKeyFrames.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    for (KeyFrameT *pKFi : pKF->GetVectorCovisibleKeyFrames()) {
        pKFi->mnBALocalForKF = pKF->mnId;
        if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
    }
    // local map points: everything the local keyframes see (:514-535)
    std::list<MapPointT *> lLocalMapPoints;
    for (KeyFrameT *pKFi : lLocalKeyFrames)
        for (MapPointT *pMP : pKFi->GetMapPointMatches())
            if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) {
                lLocalMapPoints.push_back(pMP);
                pMP->mnBALocalForKF = pKF->mnId;
            }
    // fixed keyframes: see local points without being local (:537-562)
    std::list<KeyFrameT *> lFixedKFs;
    for (MapPointT *pMP : lLocalMapPoints)
        for (const auto &ob : pMP->GetObservations()) {
            KeyFrameT *pKFi = ob.first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad()) lFixedKFs.push_back(pKFi);
            }
        }
    // vertices -> arrays (:577-618): local keyframes first (keyframe 0 of the map is held fixed), then the fixed ones
    for (KeyFrameT *k : lLocalKeyFrames) P.add_pose(k, k->mnId == 0);
    for (KeyFrameT *k : lFixedKFs) P.add_pose(k, true);
    // points and edges (:646-755)
    int pointIndex = 0;
    for (MapPointT *pMP : lLocalMapPoints) {
        P.add_point(pMP);
        for (const auto &ob : pMP->GetObservations()) {
            KeyFrameT *pKFi = ob.first;
            if (pKFi->isBad()) continue;
            const auto it = P.poseIndex.find(pKFi);
            if (it == P.poseIndex.end()) continue;        // (bad keyframes never became vertices)
            P.add_edge(pKFi, pMP, ob.second, it->second, pointIndex);
        }
        ++pointIndex;
    }
    P.localKFs.assign(lLocalKeyFrames.begin(), lLocalKeyFrames.end());
    P.localPoints.assign(lLocalMapPoints.begin(), lLocalMapPoints.end());
    return P;
}

// The same problem from the resident map: one LocalMapDevice::BAWindow, then the arrays by index — no list, no std::map lookup per
// observation, no copy of an observation map.
template <class KeyFrameT, class MapPointT>
LocalBAProblem<KeyFrameT, MapPointT> gather_local_ba(LocalMapDevice<KeyFrameT, MapPointT> &dev, KeyFrameT *pKF) {
    LocalBAProblem<KeyFrameT, MapPointT> P;
    typename LocalMapDevice<KeyFrameT, MapPointT>::Window w;
    dev.BAWindow(pKF, w);
    const size_t nLocal = w.localKFs.size();
    for (KeyFrameT *k : w.localKFs) P.add_pose(k, k->mnId == 0);
    for (KeyFrameT *k : w.fixedKFs) P.add_pose(k, true);
    P.edges.reserve(w.edgePose.size()); P.edgeKF.reserve(w.edgePose.size()); P.edgeMP.reserve(w.edgePose.size());
    for (size_t i = 0; i < w.localPoints.size(); ++i) {
        MapPointT *pMP = w.localPoints[i];
        P.add_point(pMP);
        for (int64_t e = w.edgeOff[i]; e < w.edgeOff[i + 1]; ++e) {
            const size_t j = (size_t)w.edgePose[(size_t)e];
            P.add_edge(j < nLocal ? w.localKFs[j] : w.fixedKFs[j - nLocal], pMP, w.edgeIdx[(size_t)e], (int)j, (int)i);
        }
    }
    P.localKFs.swap(w.localKFs);
    P.localPoints.swap(w.localPoints);
    return P;
}

// The optimisation and what the reference writes back (Optimizer.cc:757-926)
template <class KeyFrameT, class MapPointT, class MapT>
void solve_local_ba(LocalBAProblem<KeyFrameT, MapPointT> &P, KeyFrameT *pKF, bool *pbStopFlag, MapT *pMap) {
    std::vector<double> &poses = P.poses, &points = P.points;
    const std::vector<SivoEdge> &edges = P.edges;
    const std::vector<KeyFrameT *> &edgeKF = P.edgeKF;
    const std::vector<MapPointT *> &edgeMP = P.edgeMP;
    if (pbStopFlag && *pbStopFlag) return;                                       // :757-761
    const double intr[5] = {pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf};
    std::vector<uint8_t> erase;
    double cov[36];
    bool covOk = false;
    Optimizer::LocalBundleAdjustment(poses, P.fixedPose, points, edges, intr, pbStopFlag, erase, /*covariancePose=*/0, cov, &covOk);

    // vToErase (:824-858): the monocular edges in edge order, THEN the stereo ones; a map point's isBad() is read while the list
    // is built, i.e. before anything is erased (an erasure can turn a point bad: its later entries are still erased).  Both
    // pinned against the reference's own Optimizer.cc by tests/cpp/pin_optimizer.cpp.
    std::vector<size_t> vToErase;
    for (int stereo = 0; stereo < 2; ++stereo)
        for (size_t e = 0; e < edges.size(); ++e)
            if ((edges[e].stereo != 0) == (stereo != 0) && erase[e] && !edgeMP[e]->isBad()) vToErase.push_back(e);
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                    // :860-861
    for (size_t e : vToErase) {                                                  // :863-871
        edgeKF[e]->EraseMapPointMatch(edgeMP[e]);
        edgeMP[e]->EraseObservation(edgeKF[e]);
    }
    for (KeyFrameT *k : P.localKFs) {                                            // :884-910
        k->SetPose(cv_from_se3(poses.data() + 12 * (size_t)P.poseIndex[k]));
        if (k->mnId == pKF->mnId && covOk) set_covariance(pKF, cov);
    }
    int pointIndex = 0;
    for (MapPointT *pMP : P.localPoints) {                                       // :912-925
        cv::Mat X(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) X.at<float>(r, 0) = (float)points[3 * (size_t)pointIndex + r];
        pMP->SetWorldPos(X);
        pMP->UpdateNormalAndDepth();
        ++pointIndex;
    }
}

}  // namespace optimizer_detail

// void Optimizer::LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap)
template <class KeyFrameT, class MapT>
void LocalBundleAdjustment(KeyFrameT *pKF, bool *pbStopFlag, MapT *pMap) {
    auto P = optimizer_detail::gather_local_ba(pKF);
    optimizer_detail::solve_local_ba(P, pKF, pbStopFlag, pMap);
}

// The same with the window built on the resident map (LocalMapAdapter.h) in place of the walk: dev holds the map as the last Rebuild or
// Sync left it.  For pKF->mnId == 0 every object's initial stamp already equals the id; the host walk, which reads the stamps, runs.
template <class KeyFrameT, class MapPointT, class MapT>
void LocalBundleAdjustment(LocalMapDevice<KeyFrameT, MapPointT> &dev, KeyFrameT *pKF, bool *pbStopFlag, MapT *pMap) {
    auto P = pKF->mnId == 0 ? optimizer_detail::gather_local_ba(pKF) : optimizer_detail::gather_local_ba(dev, pKF);
    optimizer_detail::solve_local_ba(P, pKF, pbStopFlag, pMap);
}

// void Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust) (Optimizer.cc:49-271)
template <class KeyFrameT, class MapPointT>
void BundleAdjustment(const std::vector<KeyFrameT *> &vpKFs, const std::vector<MapPointT *> &vpMP, int nIterations = 5,
                      bool *pbStopFlag = nullptr, const unsigned long nLoopKF = 0ul, const bool bRobust = true) {
    using namespace optimizer_detail;
    // keyframe vertices (:77-97): every keyframe that is not bad, the map's first one held fixed
    std::map<KeyFrameT *, int> poseIndex;
    std::vector<double> poses;
    std::vector<uint8_t> fixedPose;
    unsigned long maxKFid = 0;
    for (KeyFrameT *pKF : vpKFs) {
        if (pKF->isBad()) continue;
        double p[12];
        se3_from_cv(pKF->GetPose(), p);
        poseIndex[pKF] = (int)fixedPose.size();
        poses.insert(poses.end(), p, p + 12);
        fixedPose.push_back(pKF->mnId == 0 ? 1 : 0);
        if (pKF->mnId > maxKFid) maxKFid = pKF->mnId;
    }
    if (poseIndex.empty()) return;
    // map point vertices and their observations (:102-211); a point without any edge is removed again (:204-210)
    std::vector<int> pointIndex(vpMP.size(), -1);          // vbNotIncludedMP[i] <=> pointIndex[i] < 0
    std::vector<double> points;
    std::vector<SivoEdge> edges;
    int nPoints = 0;
    for (size_t i = 0; i < vpMP.size(); ++i) {
        MapPointT *pMP = vpMP[i];
        if (pMP->isBad()) continue;
        const size_t first = edges.size();
        for (const auto &ob : pMP->GetObservations()) {
            KeyFrameT *pKF = ob.first;
            if (pKF->isBad() || pKF->mnId > maxKFid) continue;
            const auto it = poseIndex.find(pKF);
            if (it == poseIndex.end()) continue;            // (no vertex of that id: g2o refuses the edge)
            edges.push_back(observation(*pKF, ob.second, it->second, nPoints));
        }
        if (edges.size() == first) continue;
        const cv::Mat Xw = pMP->GetWorldPos();
        for (int r = 0; r < 3; ++r) points.push_back(Xw.at<float>(r, 0));
        pointIndex[i] = nPoints++;
    }
    KeyFrameT *any = poseIndex.begin()->first;
    const double intr[5] = {any->fx, any->fy, any->cx, any->cy, any->mbf};
    if (!edges.empty()) Optimizer::BundleAdjustment(poses, fixedPose, points, edges, intr, nIterations, pbStopFlag, bRobust);   // :214-217
    // keyframes (:219-235)
    for (KeyFrameT *pKF : vpKFs) {
        if (pKF->isBad()) continue;
        const cv::Mat T = cv_from_se3(poses.data() + 12 * (size_t)poseIndex[pKF]);
        if (nLoopKF == 0) {
            pKF->SetPose(T);
        } else {
            pKF->mTcwGBA = T.clone();
            pKF->mnBAGlobalForKF = nLoopKF;
        }
    }
    // points (:237-260)
    for (size_t i = 0; i < vpMP.size(); ++i) {
        if (pointIndex[i] < 0) continue;
        MapPointT *pMP = vpMP[i];
        if (pMP->isBad()) continue;
        cv::Mat X(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) X.at<float>(r, 0) = (float)points[3 * (size_t)pointIndex[i] + r];
        if (nLoopKF == 0) {
            pMP->SetWorldPos(X);
            pMP->UpdateNormalAndDepth();
        } else {
            pMP->mPosGBA = X.clone();
            pMP->mnBAGlobalForKF = nLoopKF;
        }
    }
}

// void Optimizer::GlobalBundleAdjustment(Map *pMap, nIterations, pbStopFlag, nLoopKF, bRobust) (Optimizer.cc:37-47)
template <class MapT>
void GlobalBundleAdjustment(MapT *pMap, int nIterations = 5, bool *pbStopFlag = nullptr, const unsigned long nLoopKF = 0ul,
                            const bool bRobust = true) {
    const auto vpKFs = pMap->GetAllKeyFrames();
    const auto vpMP = pMap->GetAllMapPoints();
    BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust);
}

// the static members of class Optimizer (declared in Optimizer.h)
template <class FrameT>
int Optimizer::PoseOptimization(FrameT *pFrame) { return SIVO::PoseOptimization(pFrame); }
template <class KeyFrameT, class MapT>
void Optimizer::LocalBundleAdjustment(KeyFrameT *pKF, bool *pbStopFlag, MapT *pMap) { SIVO::LocalBundleAdjustment(pKF, pbStopFlag, pMap); }
template <class KeyFrameT, class MapPointT>
void Optimizer::BundleAdjustment(const std::vector<KeyFrameT *> &vpKF, const std::vector<MapPointT *> &vpMP, int nIterations, bool *pbStopFlag,
                                 const unsigned long nLoopKF, const bool bRobust) {
    SIVO::BundleAdjustment(vpKF, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust);
}
template <class MapT>
void Optimizer::GlobalBundleAdjustment(MapT *pMap, int nIterations, bool *pbStopFlag, const unsigned long nLoopKF, const bool bRobust) {
    SIVO::GlobalBundleAdjustment(pMap, nIterations, pbStopFlag, nLoopKF, bRobust);
}

// Loop closing: Optimizer::OptimizeEssentialGraph / OptimizeSim3 (declared in Optimizer.h).  With -DSIVO_HAVE_G2O both go to the
// backend; otherwise OptimizeSim3 runs on the device under -DSIVO_SIM3_ON_DEVICE and OptimizeEssentialGraph under
// -DSIVO_ESSENTIAL_GRAPH_ON_DEVICE, and what is left is a compile-time error.
#ifdef SIVO_HAVE_G2O
template <class MapT, class KeyFrameT, class KFPoseMapT, class ConnectionsT>
void Optimizer::OptimizeEssentialGraph(MapT *pMap, KeyFrameT *pLoopKF, KeyFrameT *pCurKF, const KFPoseMapT &NonCorrectedSim3, const KFPoseMapT &CorrectedSim3,
                                       const ConnectionsT &LoopConnections, const bool &bFixScale) {
    SIVO_G2O_BACKEND::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale);
}
template <class KeyFrameT, class MapPointT, class Sim3T>
int Optimizer::OptimizeSim3(KeyFrameT *pKF1, KeyFrameT *pKF2, std::vector<MapPointT *> &vpMatches1, Sim3T &g2oS12, const float th2, const bool bFixScale) {
    return SIVO_G2O_BACKEND::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale);
}
#else
#ifdef SIVO_ESSENTIAL_GRAPH_ON_DEVICE
template <class MapT, class KeyFrameT, class KFPoseMapT, class ConnectionsT>
void Optimizer::OptimizeEssentialGraph(MapT *pMap, KeyFrameT *pLoopKF, KeyFrameT *pCurKF, const KFPoseMapT &NonCorrectedSim3, const KFPoseMapT &CorrectedSim3,
                                       const ConnectionsT &LoopConnections, const bool &bFixScale) {
    SIVO::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale);
}
#else
template <class MapT, class KeyFrameT, class KFPoseMapT, class ConnectionsT>
void Optimizer::OptimizeEssentialGraph(MapT *, KeyFrameT *, KeyFrameT *, const KFPoseMapT &, const KFPoseMapT &, const ConnectionsT &, const bool &) {
    static_assert(sizeof(MapT) == 0, "Optimizer::OptimizeEssentialGraph (Sim3 pose graph, g2o) is outside this library: build with -DSIVO_HAVE_G2O and "
                                     "-DSIVO_G2O_BACKEND=<a class providing it, e.g. the reference's Optimizer.cc compiled under another name>, "
                                     "or with -DSIVO_ESSENTIAL_GRAPH_ON_DEVICE (this library's kernels)");
}
#endif
#ifdef SIVO_SIM3_ON_DEVICE
template <class KeyFrameT, class MapPointT, class Sim3T>
int Optimizer::OptimizeSim3(KeyFrameT *pKF1, KeyFrameT *pKF2, std::vector<MapPointT *> &vpMatches1, Sim3T &g2oS12, const float th2, const bool bFixScale) {
    return SIVO::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale);
}
#else
template <class KeyFrameT, class MapPointT, class Sim3T>
int Optimizer::OptimizeSim3(KeyFrameT *, KeyFrameT *, std::vector<MapPointT *> &, Sim3T &, const float, const bool) {
    static_assert(sizeof(KeyFrameT) == 0, "Optimizer::OptimizeSim3 (Sim3 alignment, g2o) is outside this library: build with -DSIVO_HAVE_G2O and "
                                          "-DSIVO_G2O_BACKEND=<a class providing it>, or with -DSIVO_SIM3_ON_DEVICE (this library's kernel)");
    return 0;
}
#endif
#endif

}  // namespace SIVO
#endif
