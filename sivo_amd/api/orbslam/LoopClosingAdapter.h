// The two map corrections of the loop closer over the SLAM object graph:
//     void CorrectLoopPoses(pCurrentKF, g2oScw, vpCurrentConnectedKFs, CorrectedSim3, NonCorrectedSim3)
//                                              LoopClosing::CorrectLoop, reference src/orbslam/LoopClosing.cc:439-522
//     void PropagateGlobalBA(pMap, nLoopKF)    the map update of LoopClosing::RunGlobalBundleAdjustment, LoopClosing.cc:694-753
// as header-only templates.  Each gathers the arrays of include/sivo_hip.h from the object graph, makes ONE call (sivo_loop_correct /
// sivo_gba_propagate: the arithmetic runs on the device and equals the reference's loops bit for bit) and writes back what
// the reference's loops write.  The caller holds pMap->mMutexMapUpdate around either, as the reference does (:445, :692).
//
// CorrectLoopPoses fills CorrectedSim3 and NonCorrectedSim3 (empty on entry), moves every map point of the connected keyframes once
// (SetWorldPos, mnCorrectedByKF, mnCorrectedReference, the normal and the distances of UpdateNormalAndDepth) and gives every connected
// keyframe its corrected pose (SetPose).  KeyFrame::UpdateConnections of :525 is not part of it: SIVO::UpdateConnections(vpKFs) of
// CovisibilityAdapter.h does all of them in one launch afterwards.  vpCurrentConnectedKFs is mvpCurrentConnectedKFs, the current keyframe
// included (:437).  PropagateGlobalBA leaves Map::InformNewBigChange (:755) to the caller.
//
// KeyFrame, MapPoint, Map and g2o::Sim3 are template parameters (SLAM data model, outside this library — SURVEY.md 8).  The members read
// are the reference's (KeyFrame: mnId, GetPose, GetPoseInverse, GetCameraCenter, GetMapPointMatches, GetChildren, SetPose, mTcwGBA,
// mTcwBefGBA, mnBAGlobalForKF, mvKeysSemantic, mvScaleFactors, mnScaleLevels; MapPoint: isBad, GetWorldPos, SetWorldPos, GetObservations,
// GetReferenceKeyFrame, mnCorrectedByKF, mnCorrectedReference, mPosGBA, mnBAGlobalForKF; Map: GetAllKeyFrames, GetAllMapPoints,
// mvpKeyFrameOrigins), plus the setter LocalMappingAdapter.h names for what UpdateNormalAndDepth assigns under the point's mutex:
//     void SetNormalAndDepth(const cv::Mat &normal, float maxDistance, float minDistance);
#ifndef SIVO_AMD_API_LOOPCLOSINGADAPTER_H
#define SIVO_AMD_API_LOOPCLOSINGADAPTER_H

#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "OptimizerAdapter.h"

namespace SIVO {
namespace loop_closing_detail {

inline void check(int rc, const char *what) {
    if (rc == SIVO_ERR_INVALID_ARGUMENT) throw std::invalid_argument(std::string(what) + ": " + sivo_last_error());
    if (rc != SIVO_OK) throw std::runtime_error(std::string(what) + ": " + sivo_last_error());
}

// a 4 x 4 (or 3 x 1) CV_32F matrix into n floats; an empty matrix (a member never assigned) reads as zeros
inline void put_mat(const cv::Mat &M, int rows, int cols, std::vector<float> &out) {
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) out.push_back(M.empty() ? 0.0f : M.at<float>(r, c));
}
inline cv::Mat mat_of(const float *v, int rows, int cols) {
    cv::Mat M(rows, cols, CV_32F);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) M.at<float>(r, c) = v[cols * r + c];
    return M;
}

template <class Sim3T>
Sim3T sim3_of(const Sim3T &like, const double v[8]) {
    typename std::decay<decltype(like.rotation())>::type r = like.rotation();
    typename std::decay<decltype(like.translation())>::type t = like.translation();
    optimizer_detail::sim3_rot_set(r, v, 0);
    for (int i = 0; i < 3; ++i) t[i] = v[4 + i];
    return Sim3T(r, t, v[7]);
}

// dense indices in the order of first mention
template <class T>
struct Index {
    std::map<T *, int32_t> of;
    std::vector<T *> all;
    int32_t get(T *p) {
        auto it = of.find(p);
        if (it != of.end()) return it->second;
        const int32_t i = (int32_t)all.size();
        of[p] = i;
        all.push_back(p);
        return i;
    }
};

}  // namespace loop_closing_detail

template <class KeyFrameT, class Sim3T, class KFPoseMapT>
void CorrectLoopPoses(KeyFrameT *pCurrentKF, const Sim3T &g2oScw, const std::vector<KeyFrameT *> &vpCurrentConnectedKFs, KFPoseMapT &CorrectedSim3,
                      KFPoseMapT &NonCorrectedSim3) {
    using namespace loop_closing_detail;
    typedef typename std::remove_pointer<typename std::decay<decltype(pCurrentKF->GetMapPointMatches())>::type::value_type>::type MapPointT;
    // CorrectedSim3's keys in the order the reference walks them (:476): a std::map over the pointers
    const std::set<KeyFrameT *> corrected(vpCurrentConnectedKFs.begin(), vpCurrentConnectedKFs.end());
    if (!corrected.count(pCurrentKF)) throw std::invalid_argument("CorrectLoopPoses: the current keyframe is not among the connected keyframes");
    Index<KeyFrameT> kfs;
    for (KeyFrameT *pKF : corrected) kfs.get(pKF);
    const size_t K = corrected.size();
    SivoLoopCorrect a{};
    std::vector<float> tiw, twc, ow, pos, level_scale, last_scale;
    std::vector<int64_t> slot_off{0}, obs_off{0};
    std::vector<int32_t> slot_point, obs_kf, ref_kf;
    std::vector<uint8_t> skip;
    Index<MapPointT> pts;
    for (KeyFrameT *pKFi : corrected) {
        put_mat(pKFi->GetPose(), 4, 4, tiw);
        const auto vpMPsi = pKFi->GetMapPointMatches();                     // (:486)
        for (MapPointT *pMPi : vpMPsi) {
            if (!pMPi) { slot_point.push_back(-1); continue; }
            const size_t known = pts.all.size();
            const int32_t p = pts.get(pMPi);
            slot_point.push_back(p);
            if ((size_t)p < known) continue;
            const bool s = pMPi->isBad() || pMPi->mnCorrectedByKF == pCurrentKF->mnId;      // (:491-494)
            skip.push_back(s ? 1 : 0);
            float ls = 1.f, last = 1.f;
            int32_t ref = -1;
            if (s) {
                for (int r = 0; r < 3; ++r) pos.push_back(0.f);
            } else {
                put_mat(pMPi->GetWorldPos(), 3, 1, pos);
                auto observations = pMPi->GetObservations();                // in the order UpdateNormalAndDepth walks them (MapPoint.cc:391)
                for (auto mit = observations.begin(); mit != observations.end(); ++mit) obs_kf.push_back(kfs.get(mit->first));
                KeyFrameT *pRefKF = pMPi->GetReferenceKeyFrame();
                ref = pRefKF ? kfs.get(pRefKF) : 0;
                if (!observations.empty() && pRefKF) {                      // (MapPoint.cc:399-408)
                    const int level = pRefKF->mvKeysSemantic[observations[pRefKF]].octave;
                    ls = pRefKF->mvScaleFactors[level];
                    last = pRefKF->mvScaleFactors[pRefKF->mnScaleLevels - 1];
                }
            }
            ref_kf.push_back(ref);
            level_scale.push_back(ls); last_scale.push_back(last);
            obs_off.push_back((int64_t)obs_kf.size());
        }
        slot_off.push_back((int64_t)slot_point.size());
    }
    for (KeyFrameT *pKF : kfs.all) put_mat(pKF->GetCameraCenter(), 3, 1, ow);
    put_mat(pCurrentKF->GetPoseInverse(), 4, 4, twc);                       // (:441)
    const optimizer_detail::HostSim3 Scw = optimizer_detail::host_sim3_of(g2oScw);
    double scw[8];
    optimizer_detail::host_sim3_store(Scw, scw);
    const size_t P = pts.all.size();
    std::vector<double> non(8 * K), cor(8 * K);
    std::vector<float> tiw_out(16 * K), ow_out(3 * K), pos_out(3 * P), normal(3 * P), maxd(P), mind(P);
    std::vector<int32_t> by(P);
    std::vector<uint8_t> flags(P);
    a.n_kf = (int32_t)K; a.cur = kfs.of[pCurrentKF]; a.n_all = (int32_t)kfs.all.size(); a.n_points = (int32_t)P;
    a.tiw = tiw.data(); a.twc_cur = twc.data(); a.scw = scw; a.ow = ow.data(); a.slot_off = slot_off.data(); a.slot_point = slot_point.data();
    a.pos = pos.data(); a.skip = skip.data(); a.obs_off = obs_off.data(); a.obs_kf = obs_kf.data(); a.ref_kf = ref_kf.data();
    a.level_scale = level_scale.data(); a.last_scale = last_scale.data();
    a.noncorrected_siw = non.data(); a.corrected_siw = cor.data(); a.tiw_out = tiw_out.data(); a.ow_out = ow_out.data();
    a.corrected_by = by.data(); a.pos_out = pos_out.data(); a.normal = normal.data(); a.max_dist = maxd.data(); a.min_dist = mind.data();
    a.flags = flags.data();
    check(sivo_loop_correct(&a), "CorrectLoopPoses");
    for (size_t p = 0; p < P; ++p) {                                        // (:505-508)
        if (by[p] < 0) continue;
        MapPointT *pMP = pts.all[p];
        pMP->SetWorldPos(mat_of(&pos_out[3 * p], 3, 1));
        pMP->mnCorrectedByKF = pCurrentKF->mnId;
        pMP->mnCorrectedReference = kfs.all[(size_t)by[p]]->mnId;
        if (flags[p] & SIVO_MP_NO_OBSERVATION) continue;                    // as RefreshMapPoints writes them
        pMP->SetNormalAndDepth(mat_of(&normal[3 * p], 3, 1), maxd[p], mind[p]);
    }
    for (size_t i = 0; i < K; ++i) {
        KeyFrameT *pKFi = kfs.all[i];
        if (pKFi == pCurrentKF) CorrectedSim3[pKFi] = g2oScw;               // (:440) verbatim
        else CorrectedSim3[pKFi] = sim3_of(g2oScw, &cor[8 * i]);
        NonCorrectedSim3[pKFi] = sim3_of(g2oScw, &non[8 * i]);
        pKFi->SetPose(mat_of(&tiw_out[16 * i], 4, 4));                      // (:520-522)
    }
}

template <class MapT>
void PropagateGlobalBA(MapT *pMap, unsigned long nLoopKF) {
    using namespace loop_closing_detail;
    const auto vpKFs = pMap->GetAllKeyFrames();
    const auto vpMPs = pMap->GetAllMapPoints();
    typedef typename std::remove_pointer<typename std::decay<decltype(vpKFs)>::type::value_type>::type KeyFrameT;
    typedef typename std::remove_pointer<typename std::decay<decltype(vpMPs)>::type::value_type>::type MapPointT;
    Index<KeyFrameT> kfs;
    for (KeyFrameT *pKF : vpKFs) kfs.get(pKF);
    std::vector<int32_t> origin, ref_kf;
    for (KeyFrameT *pKF : pMap->mvpKeyFrameOrigins) origin.push_back(kfs.get(pKF));
    std::vector<float> pos, pos_gba;
    std::vector<uint8_t> pin, pbad;
    for (MapPointT *pMP : vpMPs) {
        const bool bad = pMP->isBad();
        put_mat(bad ? cv::Mat() : pMP->GetWorldPos(), 3, 1, pos);
        put_mat(pMP->mPosGBA, 3, 1, pos_gba);
        pin.push_back(pMP->mnBAGlobalForKF == nLoopKF ? 1 : 0);
        pbad.push_back(bad ? 1 : 0);
        KeyFrameT *pRefKF = bad ? nullptr : pMP->GetReferenceKeyFrame();
        ref_kf.push_back(pRefKF ? kfs.get(pRefKF) : -1);
    }
    // the children of every keyframe met, the list growing as they are met (a keyframe the map no longer lists may still be a child)
    std::vector<int64_t> child_off{0};
    std::vector<int32_t> child_kf;
    for (size_t k = 0; k < kfs.all.size(); ++k) {
        const auto sChilds = kfs.all[k]->GetChildren();
        for (KeyFrameT *pChild : sChilds) child_kf.push_back(kfs.get(pChild));
        child_off.push_back((int64_t)child_kf.size());
    }
    const size_t K = kfs.all.size(), P = vpMPs.size();
    std::vector<float> tcw, tcw_gba, tcw_bef;
    std::vector<uint8_t> in_gba;
    for (KeyFrameT *pKF : kfs.all) {
        put_mat(pKF->GetPose(), 4, 4, tcw);
        put_mat(pKF->mTcwGBA, 4, 4, tcw_gba);
        put_mat(pKF->mTcwBefGBA, 4, 4, tcw_bef);
        in_gba.push_back(pKF->mnBAGlobalForKF == nLoopKF ? 1 : 0);
    }
    const std::vector<uint8_t> in_before = in_gba;
    std::vector<float> tcw_out(16 * K), ow_out(3 * K), pos_out(3 * P);
    std::vector<uint8_t> reached(K), status(P);
    SivoGbaPropagate a{};
    a.n_kf = (int32_t)K; a.n_origins = (int32_t)origin.size(); a.n_points = (int32_t)P;
    a.origin = origin.data(); a.child_off = child_off.data(); a.child_kf = child_kf.data(); a.tcw = tcw.data(); a.tcw_gba = tcw_gba.data();
    a.in_gba = in_gba.data(); a.tcw_bef = tcw_bef.data(); a.pos = pos.data(); a.pos_gba = pos_gba.data(); a.point_in_gba = pin.data();
    a.point_bad = pbad.data(); a.ref_kf = ref_kf.data(); a.tcw_out = tcw_out.data(); a.ow_out = ow_out.data(); a.kf_reached = reached.data();
    a.pos_out = pos_out.data(); a.point_status = status.data();
    check(sivo_gba_propagate(&a), "PropagateGlobalBA");
    for (size_t k = 0; k < K; ++k) {
        if (!reached[k]) continue;
        KeyFrameT *pKF = kfs.all[k];
        if (!in_before[k] && in_gba[k]) {                                   // (:708-710)
            pKF->mTcwGBA = mat_of(&tcw_gba[16 * k], 4, 4);
            pKF->mnBAGlobalForKF = nLoopKF;
        }
        pKF->mTcwBefGBA = pKF->GetPose();                                   // (:715-716)
        pKF->SetPose(mat_of(&tcw_out[16 * k], 4, 4));
    }
    for (size_t p = 0; p < P; ++p)                                          // (:731, :751)
        if (status[p] == SIVO_GBA_POINT_FROM_BA || status[p] == SIVO_GBA_POINT_CARRIED) vpMPs[p]->SetWorldPos(mat_of(&pos_out[3 * p], 3, 1));
}

}  // namespace SIVO

#endif
