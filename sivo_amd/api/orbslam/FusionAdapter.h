// The two places where the SLAM threads fuse duplicated map points keyframe by keyframe, each as ONE device search and a host replay:
//     std::vector<int> FuseIntoKeyFrames(vpTargetKFs, vpMapPoints, th = 3.0f)
//         for (pKFi : vpTargetKFs) matcher.Fuse(pKFi, vpMapPoints, th)       LocalMapping::SearchInNeighbors, reference LocalMapping.cc:586-594
//     std::vector<int> SearchAndFuse(CorrectedPosesMap, vpLoopMapPoints, pMap, th = 4.0f)
//         LoopClosing::SearchAndFuse, LoopClosing.cc:609-635: matcher.Fuse(pKF, cvScw, vpLoopMapPoints, th, vpReplacePoints) for every
//         keyframe of the map in the map's order, each followed by the Replace loop under pMap->mMutexMapUpdate
// as header-only templates over the SLAM types, in the manner of CovisibilityAdapter.h.  Both return the per-keyframe nFused.
//
// Why one search serves the whole loop.  Which keypoint of keyframe k a point would fuse with depends on the keyframe's
// pose, intrinsics and keys and on the point's position, normal, distances and descriptor.  Nothing in the two loops moves a position, a
// normal or a distance (Replace, MapPoint.cc:225-261, and AddObservation do not touch them); what the surgery of the earlier keyframes
// does change is (a) whether the pair is skipped at all — isBad(), IsInKeyFrame(pKF) / spAlreadyFound — and (b) the descriptor of a
// point that survived a Replace (ComputeDistinctiveDescriptors, MapPoint.cc:258).  So:
//   1. speculate: sivo_fuse_batch over all keyframes x all points with the descriptors as they stand, masking the points that are null
//      or bad and the pairs whose point is in the keyframe at the start (such a point leaves the keyframe only by being replaced, and
//      then it is bad);
//   2. for keyframe k = 0 .. K-1, in the reference's order: compare GetDescriptor() of every point that is not bad with the bytes last
//      uploaded for it; if any differ, ONE repair call for those points x keyframes k .. K-1 overwrites their rows and snapshots;
//   3. run keyframe k's surgery exactly as the single-keyframe ORBmatcher::Fuse members do, reading isBad(), IsInKeyFrame() /
//      GetMapPoints() and GetMapPoint(best) at that moment.
// With no replacement that changes a descriptor the whole loop is one device call; with many, at most one more per keyframe.
//
// Beside what ORBmatcher.h reads, MapPoint needs the two getters TrackingAdapter.h asks for (GetMinDistance / GetMaxDistance: mfMinDistance
// and mfMaxDistance under the point's mutex) and KeyFrame mfLogScaleFactor and mnScaleLevels (the reference's KeyFrame has both).  The
// call holds every target keyframe's device view for its duration; LoopClosing stops LocalMapping before it corrects a loop
// (LoopClosing.cc:411-429), so the two adapters never run side by side, and every other matcher call holds one view at a time.
#ifndef SIVO_AMD_API_FUSIONADAPTER_H
#define SIVO_AMD_API_FUSIONADAPTER_H

#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "ORBmatcher.h"

namespace SIVO {
namespace fusion_detail {

inline void check(int rc, const char *what) {
    if (rc == SIVO_ERR_INVALID_ARGUMENT) throw std::invalid_argument(std::string(what) + ": " + sivo_last_error());
    if (rc != SIVO_OK) throw std::runtime_error(std::string(what) + ": " + sivo_last_error());
}

// TEST ONLY: false leaves the rows of a point whose descriptor changed as the first search made them (tests/test_fuse_batch_host.py
// shows with it that its scenes depend on the repair step).
inline bool &repair_switch() {
    static bool on = true;
    return on;
}

template <class KeyFrameT>
SivoFuseCamera camera_of(KeyFrameT *pKF, const matcher_detail::Pose &T, const float Ow[3], int scw_variant) {
    SivoFuseCamera c;
    for (int i = 0; i < 9; ++i) c.Rcw[i] = T.R[i];
    for (int i = 0; i < 3; ++i) { c.tcw[i] = T.t[i]; c.Ow[i] = Ow[i]; }
    c.fx = pKF->fx; c.fy = pKF->fy; c.cx = pKF->cx; c.cy = pKF->cy; c.bf = pKF->mbf;
    c.min_x = (float)pKF->mnMinX; c.max_x = (float)pKF->mnMaxX; c.min_y = (float)pKF->mnMinY; c.max_y = (float)pKF->mnMaxY;
    c.log_scale_factor = pKF->mfLogScaleFactor;
    c.nlevels = (int32_t)pKF->mnScaleLevels;
    c.scw_variant = scw_variant;
    return c;
}

// The speculative search and its repairs: best(k, i) is the keypoint of keyframe k that point i would fuse with by the descriptor the
// point has when keyframe k's turn comes (after refresh(k)).
template <class KeyFrameT, class MapPointT>
class Speculation {
 public:
    // in_keyframe(k, pMP): the point is in keyframe k now (IsInKeyFrame / spAlreadyFound)
    template <class InKeyFrame>
    Speculation(const std::vector<KeyFrameT *> &kfs, const std::vector<SivoFuseCamera> &cams, const std::vector<MapPointT *> &pts, float th,
                InKeyFrame in_keyframe)
        : pts_(pts), cams_(cams), K_(kfs.size()), N_(pts.size()), th_(th) {
        for (KeyFrameT *pKF : kfs) {
            leases_.emplace_back(new matcher_detail::FrameLease(*pKF));
            handles_.push_back(leases_.back()->get());
        }
        pos_.assign(3 * N_, 0.f); normal_.assign(3 * N_, 0.f); min_.assign(N_, 0.f); max_.assign(N_, 0.f); desc_.assign(32 * N_, 0);
        skip_point_.assign(N_, 0); skip_pair_.assign(K_ * N_, 0);
        best_.assign(K_ * N_, -1);
        for (size_t i = 0; i < N_; ++i) {
            MapPointT *pMP = pts[i];
            if (!pMP || pMP->isBad()) { skip_point_[i] = 1; continue; }
            const cv::Mat X = pMP->GetWorldPos(), Pn = pMP->GetNormal();
            for (int c = 0; c < 3; ++c) { pos_[3 * i + c] = X.at<float>(c, 0); normal_[3 * i + c] = Pn.at<float>(c, 0); }
            min_[i] = pMP->GetMinDistance(); max_[i] = pMP->GetMaxDistance();
            matcher_detail::descriptor_row(pMP->GetDescriptor(), desc_, i);
            for (size_t k = 0; k < K_; ++k) skip_pair_[k * N_ + i] = in_keyframe(k, pMP) ? 1 : 0;
        }
        if (K_ && N_) {
            std::vector<int32_t> dist(K_ * N_);
            std::vector<uint8_t> status(K_ * N_);
            check(sivo_fuse_batch(handles_.data(), cams_.data(), (int)K_, (int)N_, pos_.data(), normal_.data(), min_.data(), max_.data(),
                                  desc_.data(), skip_point_.data(), skip_pair_.data(), th_, best_.data(), dist.data(), status.data(), nullptr,
                                  nullptr, nullptr, nullptr),
                  "sivo_fuse_batch");
        }
    }

    // Before keyframe k's surgery: the points whose descriptor is no longer the one that was uploaded search keyframes k .. K-1 again.
    void refresh(size_t k) {
        std::vector<size_t> dirty;
        std::vector<uint8_t> now(32);
        for (size_t i = 0; i < N_; ++i) {
            MapPointT *pMP = pts_[i];
            if (skip_point_[i] || pMP->isBad()) continue;
            matcher_detail::descriptor_row(pMP->GetDescriptor(), now, 0);
            if (std::memcmp(now.data(), desc_.data() + 32 * i, 32) == 0) continue;
            dirty.push_back(i);
            if (repair_switch()) std::memcpy(desc_.data() + 32 * i, now.data(), 32);
        }
        if (dirty.empty() || !repair_switch()) return;
        ++repairs_;
        const size_t D = dirty.size(), R = K_ - k;
        std::vector<float> pos(3 * D), normal(3 * D), mn(D), mx(D);
        std::vector<uint8_t> desc(32 * D), skip(R * D), status(R * D);
        std::vector<int32_t> best(R * D), dist(R * D);
        for (size_t j = 0; j < D; ++j) {
            const size_t i = dirty[j];
            std::memcpy(&pos[3 * j], &pos_[3 * i], 12); std::memcpy(&normal[3 * j], &normal_[3 * i], 12);
            mn[j] = min_[i]; mx[j] = max_[i];
            std::memcpy(&desc[32 * j], &desc_[32 * i], 32);
            for (size_t r = 0; r < R; ++r) skip[r * D + j] = skip_pair_[(k + r) * N_ + i];
        }
        check(sivo_fuse_batch(handles_.data() + k, cams_.data() + k, (int)R, (int)D, pos.data(), normal.data(), mn.data(), mx.data(), desc.data(),
                              nullptr, skip.data(), th_, best.data(), dist.data(), status.data(), nullptr, nullptr, nullptr, nullptr),
              "sivo_fuse_batch");
        for (size_t j = 0; j < D; ++j)
            for (size_t r = 0; r < R; ++r) best_[(k + r) * N_ + dirty[j]] = best[r * D + j];
    }

    int32_t best(size_t k, size_t i) const { return best_[k * N_ + i]; }
    int repairs() const { return repairs_; }

 private:
    const std::vector<MapPointT *> &pts_;
    const std::vector<SivoFuseCamera> &cams_;
    size_t K_, N_;
    float th_;
    std::vector<std::unique_ptr<matcher_detail::FrameLease> > leases_;
    std::vector<sivo_mframe_t> handles_;
    std::vector<float> pos_, normal_, min_, max_;
    std::vector<uint8_t> desc_, skip_point_, skip_pair_;
    std::vector<int32_t> best_;
    int repairs_ = 0;
};

struct AsCvMat {         // the pose map's values as the 4 x 4 CV_32F Scw: a cv::Mat is one already
    const cv::Mat &operator()(const cv::Mat &S) const { return S; }
};

// how many repair calls the last adapter call of this thread made (tools/fuse_batch_probe.py and the tests read it)
inline int &last_repairs() {
    static thread_local int n = 0;
    return n;
}

}  // namespace fusion_detail

// for (pKFi : vpTargetKFs) matcher.Fuse(pKFi, vpMapPoints, th); the nFused of every keyframe.
template <class KeyFrameT, class MapPointT>
std::vector<int> FuseIntoKeyFrames(const std::vector<KeyFrameT *> &vpTargetKFs, const std::vector<MapPointT *> &vpMapPoints, const float th = 3.0f) {
    using namespace fusion_detail;
    const size_t K = vpTargetKFs.size(), N = vpMapPoints.size();
    std::vector<SivoFuseCamera> cams;
    for (KeyFrameT *pKF : vpTargetKFs) {
        const matcher_detail::Pose Tcw(pKF->GetRotation(), pKF->GetTranslation());
        const cv::Mat OwM = pKF->GetCameraCenter();
        const float Ow[3] = {OwM.at<float>(0, 0), OwM.at<float>(1, 0), OwM.at<float>(2, 0)};
        cams.push_back(camera_of(pKF, Tcw, Ow, 0));
    }
    Speculation<KeyFrameT, MapPointT> spec(vpTargetKFs, cams, vpMapPoints, th,
                                           [&](size_t k, MapPointT *pMP) { return pMP->IsInKeyFrame(vpTargetKFs[k]); });
    std::vector<int> vnFused(K, 0);
    for (size_t k = 0; k < K; ++k) {
        KeyFrameT *pKF = vpTargetKFs[k];
        spec.refresh(k);
        // ORBmatcher::Fuse's surgery (ORBmatcher.cc:909-926) in the list's order, the tests of :808-812 at this moment
        int nFused = 0;
        for (size_t i = 0; i < N; ++i) {
            const int32_t best = spec.best(k, i);
            if (best < 0) continue;
            MapPointT *pMP = vpMapPoints[i];
            if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
            ++nFused;
            MapPointT *pMPinKF = pKF->GetMapPoint(best);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
                    else pMPinKF->Replace(pMP);
                }
            } else {
                pMP->AddObservation(pKF, best);
                pKF->AddMapPoint(pMP, best);
            }
        }
        vnFused[k] = nFused;
    }
    last_repairs() = spec.repairs();
    return vnFused;
}

// LoopClosing::SearchAndFuse.  to_cv(mit->second) is the keyframe's corrected Scw as a 4 x 4 CV_32F matrix: the default takes a map of
// cv::Mat; for the reference's KeyFrameAndPose pass [](const g2o::Sim3 &S) { return Converter::toCvMat(S); }.
template <class PoseMapT, class MapPointT, class MapT, class ToCvMat = fusion_detail::AsCvMat>
std::vector<int> SearchAndFuse(const PoseMapT &CorrectedPosesMap, const std::vector<MapPointT *> &vpLoopMapPoints, MapT *pMap, const float th = 4.0f,
                               ToCvMat to_cv = ToCvMat()) {
    using namespace fusion_detail;
    typedef typename std::remove_pointer<typename PoseMapT::key_type>::type KeyFrameT;
    std::vector<KeyFrameT *> kfs;
    std::vector<SivoFuseCamera> cams;
    for (auto mit = CorrectedPosesMap.begin(); mit != CorrectedPosesMap.end(); ++mit) {
        const cv::Mat Scw = to_cv(mit->second);
        const matcher_detail::Pose Tcw(Scw, matcher_detail::sim3_scale(Scw));
        float Ow[3];
        Tcw.centre(Ow);
        kfs.push_back(mit->first);
        cams.push_back(camera_of(mit->first, Tcw, Ow, 1));
    }
    const size_t K = kfs.size(), N = vpLoopMapPoints.size();
    std::vector<std::set<MapPointT *> > found0(K);
    for (size_t k = 0; k < K; ++k) found0[k] = kfs[k]->GetMapPoints();
    Speculation<KeyFrameT, MapPointT> spec(kfs, cams, vpLoopMapPoints, th, [&](size_t k, MapPointT *pMP) { return found0[k].count(pMP) != 0; });
    std::vector<int> vnFused(K, 0);
    for (size_t k = 0; k < K; ++k) {
        KeyFrameT *pKF = kfs[k];
        spec.refresh(k);
        const std::set<MapPointT *> spAlreadyFound = pKF->GetMapPoints();                    // ORBmatcher.cc:951
        std::vector<MapPointT *> vpReplacePoints(N, static_cast<MapPointT *>(nullptr));      // LoopClosing.cc:621-622
        int nFused = 0;
        for (size_t i = 0; i < N; ++i) {
            const int32_t best = spec.best(k, i);
            if (best < 0) continue;
            MapPointT *pMP = vpLoopMapPoints[i];
            if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;                         // :962
            ++nFused;
            MapPointT *pMPinKF = pKF->GetMapPoint(best);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) vpReplacePoints[i] = pMPinKF;
            } else {
                pMP->AddObservation(pKF, best);
                pKF->AddMapPoint(pMP, best);
            }
        }
        vnFused[k] = nFused;
        std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                            // LoopClosing.cc:625-633
        for (size_t i = 0; i < N; ++i)
            if (vpReplacePoints[i]) vpReplacePoints[i]->Replace(vpLoopMapPoints[i]);
    }
    last_repairs() = spec.repairs();
    return vnFused;
}

}  // namespace SIVO
#endif
