// covis_standins.hpp — stand-in SLAM types for tests/covis_adapter_prog.cpp: KeyFrame, MapPoint and Frame with the members
// sivo_amd/api/orbslam/CovisibilityAdapter.h reads and writes, and — the yardstick of that program — the reference's own way through the same
// bookkeeping: KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles / SetBadFlag (reference src/orbslam/KeyFrame.cc:171-205,
// :327-415, :477-568 without the spanning-tree repair), MapPoint::AddObservation / EraseObservation / SetBadFlag (MapPoint.cc:149-217), and the
// loops of LocalMapping::KeyFrameCulling (LocalMapping.cc:727-792), LocalMapping::MapPointCulling (:165-196) and the vote of
// Tracking::UpdateLocalKeyFrames (Tracking.cc:1128-1142), each with one std::map copy per point as the reference has.  No locks: one thread.
#pragma once
#include <algorithm>
#include <functional>
#include <iterator>
#include <list>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace standin {

struct KeyPoint { int octave = 0; };
class KeyFrame;

class MapPoint {
 public:
    long unsigned int mnId = 0;
    long int mnFirstKFid = 0;
    std::map<KeyFrame *, size_t> mObservations;
    int nObs = 0, mnFound = 1, mnVisible = 1;
    bool mbBad = false;

    void AddObservation(KeyFrame *pKF, size_t idx);
    void EraseObservation(KeyFrame *pKF);
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    int Observations() { return nObs; }
    void SetBadFlag();
    bool isBad() { return mbBad; }
    float GetFoundRatio() { return static_cast<float>(mnFound) / mnVisible; }
    int GetFound() { return mnFound; }
    int GetVisible() { return mnVisible; }
};

class KeyFrame {
 public:
    long unsigned int mnId = 0;
    float mThDepth = 40.f;
    std::vector<KeyPoint> mvKeysSemantic;
    std::vector<float> mvRight, mvDepth;
    std::vector<MapPoint *> mvpMapPoints;
    std::map<KeyFrame *, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    bool mbFirstConnection = true, mbNotErase = false, mbToBeErased = false, mbBad = false;
    KeyFrame *mpParent = nullptr;
    std::set<KeyFrame *> mspChildren;

    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints[idx] = static_cast<MapPoint *>(nullptr); }
    void AddChild(KeyFrame *pKF) { mspChildren.insert(pKF); }
    bool isBad() { return mbBad; }
    bool GetNotErase() { return mbNotErase; }

    // the connected keyframes as the reference orders them (KeyFrame.cc:392-398, :194-200): the (weight, pointer) pairs sorted upwards, each
    // then put in FRONT of the ones before it
    static void Ordered(const std::map<KeyFrame *, int> &weights, std::vector<KeyFrame *> &kfs, std::vector<int> &ws) {
        std::vector<std::pair<int, KeyFrame *> > pairs;
        for (const auto &kw : weights) pairs.push_back(std::make_pair(kw.second, kw.first));
        std::sort(pairs.begin(), pairs.end());
        std::list<KeyFrame *> frontKfs;
        std::list<int> frontWs;
        for (const auto &wk : pairs) { frontKfs.push_front(wk.second); frontWs.push_front(wk.first); }
        kfs.assign(frontKfs.begin(), frontKfs.end());
        ws.assign(frontWs.begin(), frontWs.end());
    }

    void UpdateBestCovisibles() { Ordered(mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, mvOrderedWeights); }    // KeyFrame.cc:185-205

    void AddConnection(KeyFrame *pKF, const int &weight) {           // KeyFrame.cc:171-183: nothing to do when the weight stands already
        auto it = mConnectedKeyFrameWeights.find(pKF);
        if (it != mConnectedKeyFrameWeights.end() && it->second == weight) return;
        mConnectedKeyFrameWeights[pKF] = weight;
        UpdateBestCovisibles();
    }

    void EraseConnection(KeyFrame *pKF) {                            // KeyFrame.cc:575-588
        if (mConnectedKeyFrameWeights.erase(pKF)) UpdateBestCovisibles();
    }

    // what CovisibilityAdapter.h asks of a KeyFrame beyond the reference's members: the assignments of KeyFrame.cc:400-414
    void SetConnections(const std::map<KeyFrame *, int> &weights, const std::vector<KeyFrame *> &ordered, const std::vector<int> &orderedWeights) {
        mConnectedKeyFrameWeights = weights;
        mvpOrderedConnectedKeyFrames = ordered;
        mvOrderedWeights = orderedWeights;
        if (!mbFirstConnection || mnId == 0) return;
        mpParent = ordered.front();
        mpParent->AddChild(this);
        mbFirstConnection = false;
    }

    // KeyFrame.cc:327-415: a copy of each point's observation map, the counter keyed by pointer, connections from weight 15 on (the
    // best one when none reaches it), the ordered lists, the parent at the first connection
    void UpdateConnections() {
        std::map<KeyFrame *, int> counter;
        const std::vector<MapPoint *> slots = mvpMapPoints;
        for (MapPoint *pMP : slots) {
            if (!pMP || pMP->isBad()) continue;
            const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
            for (const auto &ob : observations)
                if (ob.first->mnId != mnId) ++counter[ob.first];
        }
        if (counter.empty()) return;
        std::map<KeyFrame *, int> strong;                               // the pairs of weight >= th
        KeyFrame *best = nullptr;
        int bestWeight = 0;
        for (const auto &kw : counter) {                                 // pointer order: the first of equal maxima wins
            if (kw.second > bestWeight) { bestWeight = kw.second; best = kw.first; }
            if (kw.second >= 15) { strong[kw.first] = kw.second; kw.first->AddConnection(this, kw.second); }
        }
        if (strong.empty()) { strong[best] = bestWeight; best->AddConnection(this, bestWeight); }
        std::vector<KeyFrame *> kfs;
        std::vector<int> ws;
        Ordered(strong, kfs, ws);
        SetConnections(counter, kfs, ws);
    }

    // KeyFrame.cc:477-568 with the spanning tree left alone: nothing for id 0, a mark for a keyframe that must not be erased, else the
    // keyframe leaves its neighbours' connections and its points' observations
    void SetBadFlag() {
        if (mnId == 0) return;
        if (mbNotErase) { mbToBeErased = true; return; }
        for (const auto &kw : mConnectedKeyFrameWeights) kw.first->EraseConnection(this);
        for (MapPoint *pMP : mvpMapPoints)
            if (pMP) pMP->EraseObservation(this);
        mConnectedKeyFrameWeights.clear();
        mvpOrderedConnectedKeyFrames.clear();
        mbBad = true;
    }
};

// MapPoint.cc:149-162: a stereo observation weighs 2
inline void MapPoint::AddObservation(KeyFrame *pKF, size_t idx) {
    if (!mObservations.insert(std::make_pair(pKF, idx)).second) return;
    nObs += pKF->mvRight[idx] >= 0 ? 2 : 1;
}

// MapPoint.cc:164-189 (mpRefKF left alone): with two observations or fewer left the point is discarded
inline void MapPoint::EraseObservation(KeyFrame *pKF) {
    const auto it = mObservations.find(pKF);
    if (it == mObservations.end()) return;
    nObs -= pKF->mvRight[it->second] >= 0 ? 2 : 1;
    mObservations.erase(it);
    if (nObs <= 2) SetBadFlag();
}

// MapPoint.cc:201-217: the point leaves every keyframe that observed it
inline void MapPoint::SetBadFlag() {
    mbBad = true;
    std::map<KeyFrame *, size_t> obs;
    obs.swap(mObservations);
    for (const auto &ob : obs) ob.first->EraseMapPointMatch(ob.second);
}

struct Frame {
    int numSemanticKeys = 0;
    std::vector<MapPoint *> mvpMapPoints;
};

// LocalMapping.cc:727-792: per local keyframe the points it holds that are seen well enough elsewhere; SetBadFlag inside the loop
inline void RefKeyFrameCulling(KeyFrame *pCurrent, bool monocular) {
    for (KeyFrame *pKF : pCurrent->GetVectorCovisibleKeyFrames()) {
        if (pKF->mnId == 0) continue;
        const std::vector<MapPoint *> slots = pKF->GetMapPointMatches();
        int points = 0, redundant = 0;
        for (size_t i = 0; i < slots.size(); i++) {
            MapPoint *pMP = slots[i];
            if (!pMP || pMP->isBad()) continue;
            if (!monocular && (pKF->mvDepth[i] > pKF->mThDepth || pKF->mvDepth[i] < 0)) continue;
            ++points;
            if (pMP->Observations() <= 3) continue;
            const int level = pKF->mvKeysSemantic[i].octave;
            const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
            int seen = 0;
            for (const auto &ob : observations) {
                if (ob.first == pKF) continue;
                if (ob.first->mvKeysSemantic[ob.second].octave <= level + 1 && ++seen >= 3) break;
            }
            if (seen >= 3) ++redundant;
        }
        if (redundant > 0.9 * points) pKF->SetBadFlag();
    }
}

// LocalMapping.cc:165-196
inline void RefMapPointCulling(std::list<MapPoint *> &recent, KeyFrame *pCurrent, bool monocular) {
    const unsigned long int current = pCurrent->mnId;
    const int thObs = monocular ? 2 : 3;
    for (auto lit = recent.begin(); lit != recent.end();) {
        MapPoint *pMP = *lit;
        const int age = (int)current - (int)pMP->mnFirstKFid;
        bool drop = true;
        if (pMP->isBad()) {
        } else if (pMP->GetFoundRatio() < 0.25f) {
            pMP->SetBadFlag();
        } else if (age >= 2 && pMP->Observations() <= thObs) {
            pMP->SetBadFlag();
        } else if (age < 3) {
            drop = false;
        }
        lit = drop ? recent.erase(lit) : std::next(lit);
    }
}

// Tracking.cc:1128-1142
inline void RefVoteLocalKeyFrames(Frame &F, std::map<KeyFrame *, int> &counter) {
    for (int i = 0; i < F.numSemanticKeys; i++) {
        MapPoint *pMP = F.mvpMapPoints[i];
        if (!pMP) continue;
        if (pMP->isBad()) { F.mvpMapPoints[i] = nullptr; continue; }
        const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
        for (const auto &ob : observations) ++counter[ob.first];
    }
}

}  // namespace standin
