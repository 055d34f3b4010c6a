// The covisibility bookkeeping of the three SLAM threads over the SLAM object graph:
//     void UpdateConnections(pKF)                             KeyFrame::UpdateConnections, reference src/orbslam/KeyFrame.cc:327-415
//     void UpdateConnections(vpKFs)                           the same for several keyframes, one launch (LoopClosing.cc:520-526)
//     void VoteLocalKeyFrames(F, keyframeCounter)             the vote of Tracking::UpdateLocalKeyFrames, Tracking.cc:1128-1142
//     void KeyFrameCulling(pCurrentKF, bMonocular)            LocalMapping::KeyFrameCulling, LocalMapping.cc:727-792
//     void MapPointCulling(recentList, pCurrentKF, bMonocular) LocalMapping::MapPointCulling, LocalMapping.cc:165-196
// as header-only templates.  Each gathers the observation table of include/sivo_hip.h from the object graph — the walk over
// mObservations the reference does with one std::map copy per point is done once — makes ONE call to sivo_covis_count,
// sivo_keyframe_culling or sivo_mappoint_culling, and writes back as the reference does: the std::map / std::sort ties by pointer value
// are resolved here, on a std::map filled from the counts and walked in pointer order as the reference walks its own.
//
// KeyFrame, MapPoint and Frame are template parameters (SLAM data model, outside this library — SURVEY.md 8).  Beside the members the
// reference's classes have (KeyFrame: mnId, GetMapPointMatches, GetVectorCovisibleKeyFrames, AddConnection, SetBadFlag, mvKeysSemantic,
// mvRight, mvDepth, mThDepth; MapPoint: isBad, GetObservations, Observations, GetFoundRatio's mnFound / mnVisible through GetFound /
// GetVisible, mnFirstKFid, SetBadFlag; Frame: numSemanticKeys, mvpMapPoints), KeyFrame needs two members for what UpdateConnections
// assigns and KeyFrameCulling reads under mMutexConnections (KeyFrame.cc:400-414, :482):
//     void SetConnections(const std::map<KeyFrame *, int> &weights, const std::vector<KeyFrame *> &ordered, const std::vector<int> &orderedWeights);
//         // mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, mvOrderedWeights = the arguments; then, if mbFirstConnection && mnId != 0:
//         // mpParent = ordered.front(); mpParent->AddChild(this); mbFirstConnection = false
//     bool GetNotErase();         // mbNotErase
// and MapPoint the two counters GetFoundRatio divides (MapPoint.cc:279-282):
//     int GetFound();             // mnFound
//     int GetVisible();           // mnVisible
#ifndef SIVO_AMD_API_COVISIBILITYADAPTER_H
#define SIVO_AMD_API_COVISIBILITYADAPTER_H

#include <algorithm>
#include <cstdint>
#include <functional>
#include <list>
#include <map>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../../include/sivo_hip.h"

namespace SIVO {
namespace covis_detail {

inline void check(int rc, const char *what) {
    if (rc == SIVO_ERR_INVALID_ARGUMENT) throw std::invalid_argument(std::string(what) + ": " + sivo_last_error());
    if (rc != SIVO_OK) throw std::runtime_error(std::string(what) + ": " + sivo_last_error());
}

// The observation table of a set of map points: keyframes and points get dense indices in the order they are first met
template <class KeyFrameT, class MapPointT>
struct Gather {
    std::map<KeyFrameT *, int32_t> kfIndex;
    std::vector<KeyFrameT *> kfs;
    std::map<MapPointT *, int32_t> pointIndex;
    std::vector<MapPointT *> points;
    std::vector<int64_t> obsOff{0};
    std::vector<int32_t> obsKf;
    std::vector<uint8_t> obsLevel, obsStereo, pointBad;

    int32_t keyframe(KeyFrameT *pKF) {
        auto it = kfIndex.find(pKF);
        if (it != kfIndex.end()) return it->second;
        const int32_t k = (int32_t)kfs.size();
        kfIndex[pKF] = k;
        kfs.push_back(pKF);
        return k;
    }
    // -1 for a null slot; a bad point's list is not read (the reference does not read it either)
    int32_t point(MapPointT *pMP) {
        if (!pMP) return -1;
        auto it = pointIndex.find(pMP);
        if (it != pointIndex.end()) return it->second;
        const int32_t p = (int32_t)points.size();
        pointIndex[pMP] = p;
        points.push_back(pMP);
        const bool bad = pMP->isBad();
        pointBad.push_back(bad ? 1 : 0);
        if (!bad) {
            const std::map<KeyFrameT *, size_t> observations = pMP->GetObservations();
            for (auto mit = observations.begin(); mit != observations.end(); mit++) {
                KeyFrameT *pKFi = mit->first;
                obsKf.push_back(keyframe(pKFi));
                obsLevel.push_back((uint8_t)pKFi->mvKeysSemantic[mit->second].octave);
                obsStereo.push_back(pKFi->mvRight[mit->second] >= 0 ? 1 : 0);
            }
        }
        obsOff.push_back((int64_t)obsKf.size());
        return p;
    }
    SivoObsTable table() const {
        SivoObsTable t;
        t.n_kf = (int32_t)kfs.size(); t.n_points = (int32_t)points.size();
        t.obs_off = obsOff.data(); t.obs_kf = obsKf.data(); t.obs_level = obsLevel.data(); t.obs_stereo = obsStereo.data();
        t.point_bad = pointBad.data();
        return t;
    }
};

// KeyFrame::UpdateConnections from the filled counter on (KeyFrame.cc:362-414).  The counter is a std::map keyed by pointer, so the walk
// below is in pointer order as the reference's is: the first of equal maxima is the fallback.  The ordered lists fall by (weight,
// pointer): what std::sort on the (weight, KeyFrame *) pairs and a push_front of each leave.
template <class KeyFrameT>
void write_connections(KeyFrameT *pKF, const std::map<KeyFrameT *, int> &counter) {
    if (counter.empty()) return;                                    // (:363)
    std::vector<std::pair<int, KeyFrameT *> > pairs;
    KeyFrameT *best = nullptr;
    int bestWeight = 0;
    for (const auto &kw : counter) {
        if (kw.second > bestWeight) { bestWeight = kw.second; best = kw.first; }
        if (kw.second < 15) continue;                               // th (:372)
        pairs.push_back(std::make_pair(kw.second, kw.first));
        kw.first->AddConnection(pKF, kw.second);
    }
    if (pairs.empty()) {                                            // (:387-390)
        pairs.push_back(std::make_pair(bestWeight, best));
        best->AddConnection(pKF, bestWeight);
    }
    std::sort(pairs.begin(), pairs.end(), std::greater<std::pair<int, KeyFrameT *> >());
    std::vector<KeyFrameT *> ordered;
    std::vector<int> weights;
    for (const auto &wk : pairs) { ordered.push_back(wk.second); weights.push_back(wk.first); }
    pKF->SetConnections(counter, ordered, weights);                 // (:400-414)
}

}  // namespace covis_detail

// KeyFrame::UpdateConnections for every keyframe of the vector: one launch counts for all of them (the counts read only the map points'
// observations, which no UpdateConnections changes), the write-backs follow in the vector's order, so the result is that of the sequential
// calls of LoopClosing.cc:520-526.
template <class KeyFrameT>
void UpdateConnections(const std::vector<KeyFrameT *> &vpKFs) {
    if (vpKFs.empty()) return;
    typedef typename std::remove_pointer<typename decltype(std::declval<KeyFrameT>().GetMapPointMatches())::value_type>::type MapPointT;
    covis_detail::Gather<KeyFrameT, MapPointT> g;
    std::vector<int64_t> setOff{0};
    std::vector<int32_t> setPoint, setSelf;
    for (KeyFrameT *pKF : vpKFs) {
        const std::vector<MapPointT *> vpMP = pKF->GetMapPointMatches();            // (:330-335)
        for (MapPointT *pMP : vpMP) setPoint.push_back(g.point(pMP));
        setOff.push_back((int64_t)setPoint.size());
    }
    // (:356) compares mnId, not the pointer: the keyframe itself, once every observer has an index
    for (KeyFrameT *pKF : vpKFs) setSelf.push_back(g.keyframe(pKF));
    const SivoObsTable t = g.table();
    std::vector<int32_t> counts(vpKFs.size() * g.kfs.size(), 0);
    covis_detail::check(sivo_covis_count(&t, (int)vpKFs.size(), setOff.data(), setPoint.data(), setSelf.data(), counts.data()), "UpdateConnections");
    for (size_t s = 0; s < vpKFs.size(); ++s) {
        std::map<KeyFrameT *, int> KFcounter;
        const int32_t *row = counts.data() + s * g.kfs.size();
        for (size_t k = 0; k < g.kfs.size(); ++k)
            if (row[k] > 0 && g.kfs[k]->mnId != vpKFs[s]->mnId) KFcounter[g.kfs[k]] = row[k];
        covis_detail::write_connections(vpKFs[s], KFcounter);
    }
}

template <class KeyFrameT>
void UpdateConnections(KeyFrameT *pKF) {
    UpdateConnections(std::vector<KeyFrameT *>(1, pKF));
}

// The vote at the top of Tracking::UpdateLocalKeyFrames (Tracking.cc:1128-1142): keyframeCounter is filled, bad points leave the frame.
// The rest of the function is list surgery and stays with the caller.
template <class FrameT, class KeyFrameT>
void VoteLocalKeyFrames(FrameT &F, std::map<KeyFrameT *, int> &keyframeCounter) {
    typedef typename std::remove_pointer<typename decltype(F.mvpMapPoints)::value_type>::type MapPointT;
    covis_detail::Gather<KeyFrameT, MapPointT> g;
    std::vector<int32_t> setPoint;
    for (int i = 0; i < F.numSemanticKeys; i++) {
        MapPointT *pMP = F.mvpMapPoints[i];
        if (pMP && pMP->isBad()) {
            F.mvpMapPoints[i] = nullptr;                            // (:1139)
            pMP = nullptr;
        }
        setPoint.push_back(g.point(pMP));
    }
    keyframeCounter.clear();
    if (g.kfs.empty()) return;
    const std::vector<int64_t> setOff{0, (int64_t)setPoint.size()};
    const int32_t self = -1;
    const SivoObsTable t = g.table();
    std::vector<int32_t> counts(g.kfs.size(), 0);
    covis_detail::check(sivo_covis_count(&t, 1, setOff.data(), setPoint.data(), &self, counts.data()), "VoteLocalKeyFrames");
    for (size_t k = 0; k < g.kfs.size(); ++k)
        if (counts[k] > 0) keyframeCounter[g.kfs[k]] = counts[k];
}

// LocalMapping::KeyFrameCulling: the decisions of the whole loop come from one launch that reproduces its sequential effects; SetBadFlag
// then runs in order on every keyframe the loop calls it on (decision 1: culled; 2: mbNotErase, SetBadFlag only sets mbToBeErased).
template <class KeyFrameT>
void KeyFrameCulling(KeyFrameT *pCurrentKF, bool bMonocular) {
    typedef typename std::remove_pointer<typename decltype(std::declval<KeyFrameT>().GetMapPointMatches())::value_type>::type MapPointT;
    const std::vector<KeyFrameT *> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();   // (:729-730)
    if (vpLocalKeyFrames.empty()) return;
    covis_detail::Gather<KeyFrameT, MapPointT> g;
    const size_t K = vpLocalKeyFrames.size();
    std::vector<int32_t> localKf(K), slotPoint;
    std::vector<uint8_t> isId0(K), erasable(K), slotLevel;
    std::vector<float> thDepth(K), slotDepth;
    std::vector<int64_t> slotOff{0};
    for (size_t j = 0; j < K; ++j) {
        KeyFrameT *pKF = vpLocalKeyFrames[j];
        localKf[j] = g.keyframe(pKF);
        isId0[j] = pKF->mnId == 0;                                  // (:735)
        erasable[j] = !pKF->GetNotErase();                          // (KeyFrame.cc:482)
        thDepth[j] = pKF->mThDepth;
        if (!isId0[j]) {
            const std::vector<MapPointT *> vpMapPoints = pKF->GetMapPointMatches();               // (:739)
            for (size_t i = 0; i < vpMapPoints.size(); i++) {
                slotPoint.push_back(g.point(vpMapPoints[i]));
                slotLevel.push_back((uint8_t)pKF->mvKeysSemantic[i].octave);
                slotDepth.push_back(pKF->mvDepth[i]);
            }
        }
        slotOff.push_back((int64_t)slotPoint.size());
    }
    const SivoObsTable t = g.table();
    std::vector<int32_t> nMPs(K, 0), nRedundant(K, 0);
    std::vector<uint8_t> decision(K, 0), badAfter(g.points.size() + 1, 0);
    covis_detail::check(sivo_keyframe_culling(&t, (int)K, localKf.data(), isId0.data(), erasable.data(), thDepth.data(), slotOff.data(), slotPoint.data(),
                                              slotLevel.data(), slotDepth.data(), bMonocular ? 1 : 0, nMPs.data(), nRedundant.data(), decision.data(),
                                              badAfter.data()),
                        "KeyFrameCulling");
    for (size_t j = 0; j < K; ++j)
        if (decision[j] == SIVO_KFCULL_CULLED || decision[j] == SIVO_KFCULL_TO_BE_ERASED) vpLocalKeyFrames[j]->SetBadFlag();    // (:790)
}

// LocalMapping::MapPointCulling: the branch of every point of the list from one launch, then the list surgery and SetBadFlag of :179-195.
// No point's branch depends on another's: SetBadFlag of one point changes nothing the loop reads of the others (a point listed twice is
// flagged once).
template <class MapPointT, class KeyFrameT>
void MapPointCulling(std::list<MapPointT *> &lpRecentAddedMapPoints, KeyFrameT *pCurrentKF, bool bMonocular) {
    const size_t n = lpRecentAddedMapPoints.size();
    if (n == 0) return;
    std::vector<int32_t> found, visible, nObs;
    std::vector<int64_t> firstKF;
    std::vector<uint8_t> bad, status(n, 0);
    for (MapPointT *pMP : lpRecentAddedMapPoints) {
        found.push_back((int32_t)pMP->GetFound()); visible.push_back((int32_t)pMP->GetVisible());
        firstKF.push_back((int64_t)pMP->mnFirstKFid); nObs.push_back((int32_t)pMP->Observations()); bad.push_back(pMP->isBad() ? 1 : 0);
    }
    covis_detail::check(sivo_mappoint_culling((int)n, found.data(), visible.data(), firstKF.data(), nObs.data(), bad.data(), (int64_t)pCurrentKF->mnId,
                                              bMonocular ? 1 : 0, status.data()),
                        "MapPointCulling");
    auto lit = lpRecentAddedMapPoints.begin();
    for (size_t i = 0; i < n; ++i) {
        MapPointT *pMP = *lit;
        if ((status[i] == SIVO_MPCULL_FOUND_RATIO || status[i] == SIVO_MPCULL_OBSERVATIONS) && !pMP->isBad()) pMP->SetBadFlag();     // (:184, :188)
        if (status[i] == SIVO_MPCULL_STAYS) lit++;                                                                 // (:193)
        else lit = lpRecentAddedMapPoints.erase(lit);                                                              // (:182, :185, :189, :191)
    }
}

}  // namespace SIVO

#endif
