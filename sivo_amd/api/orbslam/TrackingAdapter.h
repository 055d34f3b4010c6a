// The step the tracking thread takes on every frame between its two pose optimisations, over the SLAM object graph:
//     bool isInFrustum(F, pMP, viewingCosLimit)            Frame::isInFrustum, reference src/orbslam/Frame.cc:267-324, on the host
//     int  SearchLocalPoints(F, vpLocalMapPoints, th)      Tracking::SearchLocalPoints, src/orbslam/Tracking.cc:1033-1085
//     int  TrackLocalMapSearch(dev, F, vpLocalKeyFrames, vpLocalMapPoints, pReferenceKF, th)
//                                                          UpdateLocalMap() and SearchLocalPoints() of Tracking::TrackLocalMap (:1087-1124,
//                                                          :1033-1085) in ONE call on the resident map of LocalMapAdapter.h
// as header-only templates.  SearchLocalPoints runs the reference's first loop over the frame's own points as it stands, gathers the local
// map into arrays, makes ONE call to sivo_search_local_points — the device culls every point with isInFrustum's arithmetic, writes the
// query of every point in view and runs ORBmatcher::SearchByProjection's matching on them (sivo_amd/csrc/frustum_math.hpp, search.hip) —
// and writes back what the reference leaves behind: mbTrackInView and the mTrack* fields, IncreaseVisible() of the points in view, the
// matches in F.mvpMapPoints.
//
// Frame and MapPoint are template parameters (SLAM data model, outside this library — SURVEY.md 8).  Beside the members the reference's
// classes have (Frame: mTcw, fx, fy, cx, cy, mbf, mnMinX .. mnMaxY, mfLogScaleFactor, mnScaleLevels, mnId, mvpMapPoints and what
// ORBmatcher.h reads; MapPoint: isBad, IncreaseVisible, Observations, GetWorldPos, GetNormal, GetDescriptor, mnLastFrameSeen,
// mbTrackInView, mTrackProjX, mTrackProjY, mTrackProjXR, mnTrackScaleLevel, mTrackViewCos), MapPoint needs two getters for the distances
// PredictScale and the *Invariance getters read under its own mutex (MapPoint.cc:413-453):
//     float GetMinDistance();     // mfMinDistance
//     float GetMaxDistance();     // mfMaxDistance
#ifndef SIVO_AMD_API_TRACKINGADAPTER_H
#define SIVO_AMD_API_TRACKINGADAPTER_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "LocalMapAdapter.h"
#include "ORBmatcher.h"
#include "../../csrc/frustum_math.hpp"

namespace SIVO {
namespace tracking_detail {

inline void check(int rc, const char *what) {
    if (rc == SIVO_ERR_INVALID_ARGUMENT) throw std::invalid_argument(std::string(what) + ": " + sivo_last_error());
    if (rc != SIVO_OK) throw std::runtime_error(std::string(what) + ": " + sivo_last_error());
}

// what isInFrustum reads of the frame; the pose from mTcw, as the matcher's adapters take it
template <class FrameT>
SivoFrustum frustum_of(const FrameT &F, float viewingCosLimit) {
    const matcher_detail::Pose T(F.mTcw);
    SivoFrustum f;
    for (int i = 0; i < 9; ++i) f.Rcw[i] = T.R[i];
    for (int i = 0; i < 3; ++i) f.tcw[i] = T.t[i];
    f.fx = F.fx; f.fy = F.fy; f.cx = F.cx; f.cy = F.cy; f.bf = F.mbf;
    f.min_x = (float)F.mnMinX; f.max_x = (float)F.mnMaxX; f.min_y = (float)F.mnMinY; f.max_y = (float)F.mnMaxY;
    f.log_scale_factor = F.mfLogScaleFactor;
    f.nlevels = (int32_t)F.mnScaleLevels;
    f.cos_limit = viewingCosLimit;
    return f;
}

template <class MapPointT>
void write_track(MapPointT *pMP, float u, float v, float ur, float viewCos, int level) {
    pMP->mbTrackInView = true;
    pMP->mTrackProjX = u;
    pMP->mTrackProjXR = ur;
    pMP->mTrackProjY = v;
    pMP->mnTrackScaleLevel = level;
    pMP->mTrackViewCos = viewCos;
}

template <class MapPointT>
void read_point(MapPointT *pMP, float X[3], float N[3]) {
    const cv::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal();
    for (int k = 0; k < 3; ++k) { X[k] = P.at<float>(k, 0); N[k] = Pn.at<float>(k, 0); }
}

}  // namespace tracking_detail

// Frame::isInFrustum with a camera made once (sivo::fr_camera: the level thresholds cost a few hundred logf calls)
template <class MapPointT>
bool isInFrustum(const sivo::FrCamera &cam, MapPointT *pMP) {
    pMP->mbTrackInView = false;
    float X[3], N[3];
    tracking_detail::read_point(pMP, X, N);
    sivo::FrResult o;
    if (sivo::fr_point(cam, X, N, pMP->GetMinDistance(), pMP->GetMaxDistance(), o) != SIVO_FRUSTUM_IN_VIEW) return false;
    tracking_detail::write_track(pMP, o.u, o.v, o.ur, o.view_cos, o.level);
    return true;
}

template <class FrameT, class MapPointT>
bool isInFrustum(FrameT &F, MapPointT *pMP, float viewingCosLimit) {
    sivo::FrCamera cam;
    if (!sivo::fr_camera(tracking_detail::frustum_of(F, viewingCosLimit), cam))
        throw std::invalid_argument("isInFrustum: mnScaleLevels outside 1 .. 16 or mfLogScaleFactor not positive");
    return isInFrustum(cam, pMP);
}

// Tracking::SearchLocalPoints.  th: 1, 3 for RGB-D, 5 after a recent relocalisation (Tracking.cc:1074-1082); nnratio: the matcher's
// (:1073).  Returns what SearchByProjection returns, 0 when no point is in view; *pnToMatch = nToMatch.
template <class FrameT, class MapPointT>
int SearchLocalPoints(FrameT &F, const std::vector<MapPointT *> &vpLocalMapPoints, float th, float nnratio = 0.8f, int *pnToMatch = nullptr) {
    using namespace matcher_detail;
    // Do not search map points already matched (:1035-1049)
    for (auto vit = F.mvpMapPoints.begin(), vend = F.mvpMapPoints.end(); vit != vend; vit++) {
        MapPointT *pMP = *vit;
        if (!pMP) continue;
        if (pMP->isBad()) {
            *vit = static_cast<MapPointT *>(nullptr);
        } else {
            pMP->IncreaseVisible();
            pMP->mnLastFrameSeen = F.mnId;
            pMP->mbTrackInView = false;
        }
    }
    // Project points in frame and check its visibility (:1054-1070): gathered here, culled on the device
    const size_t n = vpLocalMapPoints.size();
    std::vector<float> pos(3 * n, 0.f), normal(3 * n, 0.f), minDist(n, 0.f), maxDist(n, 0.f);
    std::vector<uint8_t> skip(n, 0), desc(32 * n, 0), status(n, 0);
    std::vector<int32_t> obs(n, 0), level(n, 0);
    std::vector<float> px(n, 0.f), py(n, 0.f), pxr(n, 0.f), viewCos(n, 0.f);
    for (size_t i = 0; i < n; ++i) {
        MapPointT *pMP = vpLocalMapPoints[i];
        if (pMP->mnLastFrameSeen == F.mnId || pMP->isBad()) { skip[i] = 1; continue; }
        tracking_detail::read_point(pMP, &pos[3 * i], &normal[3 * i]);
        minDist[i] = pMP->GetMinDistance(); maxDist[i] = pMP->GetMaxDistance();
        obs[i] = (int32_t)pMP->Observations();
        descriptor_row(pMP->GetDescriptor(), desc, i);
    }
    const SivoFrustum fr = tracking_detail::frustum_of(F, 0.5f);
    FrameLease dF(F);
    std::vector<int32_t> occ(dF.size()), match(dF.size());
    for (int k = 0; k < dF.size(); ++k) occ[k] = F.mvpMapPoints[k] ? (int32_t)F.mvpMapPoints[k]->Observations() : -1;
    int nToMatch = 0, nmatches = 0;
    tracking_detail::check(sivo_search_local_points(dF.get(), &fr, (int)n, pos.data(), normal.data(), minDist.data(), maxDist.data(), skip.data(),
                                                    desc.data(), obs.data(), th, nnratio, occ.data(), match.data(), status.data(), px.data(),
                                                    py.data(), pxr.data(), viewCos.data(), level.data(), &nToMatch, &nmatches),
                           "SearchLocalPoints");
    for (size_t i = 0; i < n; ++i) {
        MapPointT *pMP = vpLocalMapPoints[i];
        if (status[i] == SIVO_FRUSTUM_SKIPPED) continue;
        pMP->mbTrackInView = false;                                     // (Frame.cc:268)
        if (status[i] != SIVO_FRUSTUM_IN_VIEW) continue;
        tracking_detail::write_track(pMP, px[i], py[i], pxr[i], viewCos[i], level[i]);
        pMP->IncreaseVisible();
    }
    if (pnToMatch) *pnToMatch = nToMatch;
    if (nToMatch == 0) return 0;                                        // (:1072)
    for (int k = 0; k < dF.size(); ++k)
        if (match[k] >= 0) F.mvpMapPoints[k] = vpLocalMapPoints[match[k]];
    return nmatches;
}

// SIVO::UpdateLocalMap followed by SIVO::SearchLocalPoints, with every side effect of that pair in the same place — the frame's cleared
// slots, both vectors, mnTrackReferenceForFrame, pReferenceKF and F.mpReferenceKF; IncreaseVisible, mnLastFrameSeen and mbTrackInView of
// the frame's own points; mbTrackInView, the mTrack* fields and IncreaseVisible of the local points; the matches in F.mvpMapPoints —
// from ONE sivo_localmap_search_local_points: no MapPoint of the local map is read on the host, their attributes are the ones the
// handle keeps (dev.KeepAttributes() before Rebuild; Touch / TouchGeometry and Sync keep them current, and a point that moved without
// either is stale).  seen_point — the points whose mnLastFrameSeen already equals F.mnId when the call starts, such as the outliers
// dropped at Tracking.cc:626-630 — is gathered by one walk over the handle's points that reads mnLastFrameSeen, a field only the
// tracking thread writes, beside the mnTrackReferenceForFrame the update's premarks are read from.  isBad() is the handle's (MarkBad,
// Touch), as in UpdateLocalMap.  Returns what SearchByProjection returns, 0 when no point is in view; *pnToMatch = nToMatch.
template <class KeyFrameT, class MapPointT, class FrameT>
int TrackLocalMapSearch(LocalMapDevice<KeyFrameT, MapPointT> &dev, FrameT &F, std::vector<KeyFrameT *> &vpLocalKeyFrames,
                        std::vector<MapPointT *> &vpLocalMapPoints, KeyFrameT *&pReferenceKF, float th, float nnratio = 0.8f,
                        int *pnToMatch = nullptr) {
    using namespace matcher_detail;
    std::lock_guard<std::mutex> lock(dev.mMutex);                  // the whole call: it sees the map before a Sync or after it
    if (!dev.mHandle) throw std::invalid_argument("TrackLocalMapSearch: Rebuild has not run");
    if (!dev.KeepsAttributes()) throw std::invalid_argument("TrackLocalMapSearch: the device map keeps no attributes (KeepAttributes() before Rebuild)");
    localmap_detail::UpdateCall<KeyFrameT, MapPointT, FrameT> c(dev, F, vpLocalKeyFrames, "TrackLocalMapSearch");
    std::vector<int32_t> seen;
    for (size_t p = 0; p < dev.mvpPoints.size(); ++p)
        if (dev.mvpPoints[p]->mnLastFrameSeen == F.mnId) seen.push_back((int32_t)p);
    const SivoFrustum fr = tracking_detail::frustum_of(F, 0.5f);
    FrameLease dF(F);
    const size_t n = c.localPoint.size();
    std::vector<uint8_t> status(n, 0);
    std::vector<float> px(n, 0.f), py(n, 0.f), pxr(n, 0.f), viewCos(n, 0.f);
    std::vector<int32_t> level(n, 0), match((size_t)dF.size(), -1);
    int nToMatch = 0, nmatches = 0;
    tracking_detail::check(
        sivo_localmap_search_local_points(dev.mHandle, dF.get(), &fr, (int)c.framePoint.size(), c.framePoint.data(), (int)c.kfMarked.size(),
                                          c.kfMarked.data(), (int)c.pointMarked.size(), c.pointMarked.data(), (int)c.prev.size(), c.prev.data(),
                                          (int)seen.size(), seen.data(), th, nnratio, &c.voted, c.cleared.data(), (int)c.localKf.size(),
                                          c.localKf.data(), &c.nLocalKf, &c.refKf, (int)c.localPoint.size(), c.localPoint.data(), &c.nLocalPoints,
                                          nullptr, status.data(), px.data(), py.data(), pxr.data(), viewCos.data(), level.data(), match.data(),
                                          &nToMatch, &nmatches),
        "TrackLocalMapSearch");
    c.WriteBack(dev, F, vpLocalKeyFrames, vpLocalMapPoints, pReferenceKF);
    // Do not search map points already matched (:1035-1049); the slots of the bad ones are cleared already (:1139)
    for (auto vit = F.mvpMapPoints.begin(), vend = F.mvpMapPoints.end(); vit != vend; vit++) {
        MapPointT *pMP = *vit;
        if (!pMP) continue;
        pMP->IncreaseVisible();
        pMP->mnLastFrameSeen = F.mnId;
        pMP->mbTrackInView = false;
    }
    for (size_t i = 0; i < vpLocalMapPoints.size(); ++i) {                 // (:1054-1070)
        MapPointT *pMP = vpLocalMapPoints[i];
        if (status[i] == SIVO_FRUSTUM_SKIPPED) continue;
        pMP->mbTrackInView = false;                                     // (Frame.cc:268)
        if (status[i] != SIVO_FRUSTUM_IN_VIEW) continue;
        tracking_detail::write_track(pMP, px[i], py[i], pxr[i], viewCos[i], level[i]);
        pMP->IncreaseVisible();
    }
    if (pnToMatch) *pnToMatch = nToMatch;
    if (nToMatch == 0) return 0;                                        // (:1072)
    for (int k = 0; k < dF.size(); ++k)
        if (match[k] >= 0) F.mvpMapPoints[k] = vpLocalMapPoints[(size_t)match[k]];
    return nmatches;
}

}  // namespace SIVO

#endif
