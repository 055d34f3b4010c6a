// fuse_batch_standins.hpp — KeyFrame / MapPoint / Map with the reference's member names, as far as ORBmatcher::Fuse (both forms),
// SIVO::FuseIntoKeyFrames and SIVO::SearchAndFuse read and write them, for tests/fuse_batch_adapter_prog.cpp.  Test infrastructure only.
//
// Restated from the reference, line by line:
//   MapPoint::AddObservation                 MapPoint.cc:149-162
//   MapPoint::Replace                        MapPoint.cc:225-261   (with IncreaseFound / IncreaseVisible and ComputeDistinctiveDescriptors)
//   MapPoint::ComputeDistinctiveDescriptors  MapPoint.cc:284-347   (bad keyframes skipped, median index 0.5 * (N - 1))
//   MapPoint::PredictScale, the *Invariance getters   MapPoint.cc:413-437
//   KeyFrame::AddMapPoint / EraseMapPointMatch / ReplaceMapPointMatch / GetMapPoints / GetMapPoint   KeyFrame.cc:260-292, :322-325
//   KeyFrame::IsInImage                      KeyFrame.cc:638-640
//   Map::EraseMapPoint                       Map.cc:42-48
// Every mutation is appended to the event log of the graph it happens in (the kind of log oracle/ref_shims/slam_standins.h keeps), so
// that two runs on copies of one graph compare event by event.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "compat/cv_min.hpp"

namespace fuse_standins {

struct Event {
    // 0 Replace(point a -> point b), 1 AddObservation(point a, keyframe b, idx c), 2 AddMapPoint(keyframe a, idx b, point c),
    // 3 descriptor of point a taken from keyframe b, idx c, 4 Map::EraseMapPoint(point a), 5 EraseMapPointMatch(keyframe a, idx b),
    // 6 ReplaceMapPointMatch(keyframe a, idx b, point c)
    long kind, a, b, c;
};
inline std::vector<Event> *&log_of_current_graph() { static std::vector<Event> *log = nullptr; return log; }
inline void note(long kind, long a, long b, long c) { if (log_of_current_graph()) log_of_current_graph()->push_back(Event{kind, a, b, c}); }

inline int descriptor_distance(const unsigned char *a, const unsigned char *b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

class KeyFrame;
class MapPoint;

class Map {
 public:
    std::mutex mMutexMapUpdate;
    std::set<MapPoint *> mspMapPoints;
    inline void EraseMapPoint(MapPoint *pMP);
};

class KeyFrame {
 public:
    long unsigned int mnId = 0;
    std::vector<cv::KeyPoint> mvKeysSemantic;
    std::vector<float> mvRight;
    cv::Mat mDescriptorsSemantic;
    std::vector<MapPoint *> mvpMapPoints;
    cv::Mat mTcw, mOw;
    std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    int mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
    float mfLogScaleFactor = 0;
    int mnScaleLevels = 0;
    bool mbBad = false;

    bool isBad() const { return mbBad; }
    cv::Mat GetRotation() const { return mTcw.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation() const { return mTcw.rowRange(0, 3).col(3).clone(); }
    cv::Mat GetCameraCenter() const { return mOw.clone(); }
    bool IsInImage(const float &x, const float &y) const { return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY); }
    MapPoint *GetMapPoint(const size_t &idx) const { return mvpMapPoints[idx]; }
    std::vector<MapPoint *> GetMapPointMatches() const { return mvpMapPoints; }
    inline std::set<MapPoint *> GetMapPoints() const;
    inline void AddMapPoint(MapPoint *pMP, const size_t &idx);
    inline void EraseMapPointMatch(const size_t &idx);
    inline void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP);
};

class MapPoint {
 public:
    long unsigned int mnId = 0;
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance = 0, mfMaxDistance = 0;
    int nObs = 0, mnVisible = 1, mnFound = 1;
    bool mbBad = false;
    MapPoint *mpReplaced = nullptr;
    std::map<KeyFrame *, size_t> mObservations;
    Map *mpMap = nullptr;

    bool isBad() const { return mbBad; }
    int Observations() const { return nObs; }
    cv::Mat GetWorldPos() const { return mWorldPos.clone(); }
    cv::Mat GetNormal() const { return mNormalVector.clone(); }
    cv::Mat GetDescriptor() const { return mDescriptor.clone(); }
    float GetMinDistance() const { return mfMinDistance; }
    float GetMaxDistance() const { return mfMaxDistance; }
    float GetMinDistanceInvariance() const { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() const { return 1.2f * mfMaxDistance; }
    bool IsInKeyFrame(KeyFrame *pKF) const { return (mObservations.count(pKF)); }
    void IncreaseVisible(int n = 1) { mnVisible += n; }
    void IncreaseFound(int n = 1) { mnFound += n; }
    int PredictScale(const float &currentDist, KeyFrame *pKF) const {
        float ratio = mfMaxDistance / currentDist;
        int nScale = static_cast<int>(std::ceil(std::log(ratio) / pKF->mfLogScaleFactor));
        if (nScale < 0)
            nScale = 0;
        else if (nScale >= pKF->mnScaleLevels)
            nScale = pKF->mnScaleLevels - 1;
        return nScale;
    }
    void AddObservation(KeyFrame *pKF, size_t idx) {
        note(1, (long)mnId, (long)pKF->mnId, (long)idx);
        if (mObservations.count(pKF)) {
            return;
        }
        mObservations[pKF] = idx;
        if (pKF->mvRight[idx] >= 0) {
            nObs += 2;
        } else {
            nObs++;
        }
    }
    void Replace(MapPoint *pMP) {
        note(0, (long)mnId, (long)pMP->mnId, 0);
        if (pMP->mnId == this->mnId) {
            return;
        }
        int nvisible, nfound;
        std::map<KeyFrame *, size_t> obs;
        {
            obs = mObservations;
            mObservations.clear();
            mbBad = true;
            nvisible = mnVisible;
            nfound = mnFound;
            mpReplaced = pMP;
        }
        for (auto mit = obs.begin(), mend = obs.end(); mit != mend; mit++) {
            KeyFrame *pKF = mit->first;
            if (!pMP->IsInKeyFrame(pKF)) {
                pKF->ReplaceMapPointMatch(mit->second, pMP);
                pMP->AddObservation(pKF, mit->second);
            } else {
                pKF->EraseMapPointMatch(mit->second);
            }
        }
        pMP->IncreaseFound(nfound);
        pMP->IncreaseVisible(nvisible);
        pMP->ComputeDistinctiveDescriptors();
        mpMap->EraseMapPoint(this);
    }
    void ComputeDistinctiveDescriptors() {
        std::vector<cv::Mat> vDescriptors;
        std::vector<std::pair<long, long> > from;          // (keyframe id, idx) of each row, for the log
        std::map<KeyFrame *, size_t> observations;
        {
            if (mbBad) {
                return;
            }
            observations = mObservations;
        }
        if (observations.empty()) {
            return;
        }
        vDescriptors.reserve(observations.size());
        for (auto mit = observations.begin(); mit != observations.end(); mit++) {
            KeyFrame *pKF = mit->first;
            if (!pKF->isBad()) {
                vDescriptors.push_back(pKF->mDescriptorsSemantic.row((int)mit->second));
                from.push_back(std::make_pair((long)pKF->mnId, (long)mit->second));
            }
        }
        if (vDescriptors.empty())
            return;
        const size_t N = vDescriptors.size();
        std::vector<float> Distances(N * N);
        for (size_t i = 0; i < N; i++) {
            Distances[i * N + i] = 0;
            for (size_t j = i + 1; j < N; j++) {
                int distij = descriptor_distance(vDescriptors[i].ptr(0), vDescriptors[j].ptr(0));
                Distances[i * N + j] = distij;
                Distances[j * N + i] = distij;
            }
        }
        int BestMedian = INT_MAX;
        int BestIdx = 0;
        for (size_t i = 0; i < N; i++) {
            std::vector<int> vDists(Distances.begin() + (long)(i * N), Distances.begin() + (long)(i * N + N));
            std::sort(vDists.begin(), vDists.end());
            int median = vDists[(size_t)(0.5 * (N - 1))];
            if (median < BestMedian) {
                BestMedian = median;
                BestIdx = (int)i;
            }
        }
        {
            mDescriptor = vDescriptors[(size_t)BestIdx].clone();
            note(3, (long)mnId, from[(size_t)BestIdx].first, from[(size_t)BestIdx].second);
        }
    }
};

inline std::set<MapPoint *> KeyFrame::GetMapPoints() const {
    std::set<MapPoint *> s;
    for (size_t i = 0, iend = mvpMapPoints.size(); i < iend; i++) {
        if (!mvpMapPoints[i])
            continue;
        MapPoint *pMP = mvpMapPoints[i];
        if (!pMP->isBad())
            s.insert(pMP);
    }
    return s;
}
inline void KeyFrame::AddMapPoint(MapPoint *pMP, const size_t &idx) {
    note(2, (long)mnId, (long)idx, (long)pMP->mnId);
    mvpMapPoints[idx] = pMP;
}
inline void KeyFrame::EraseMapPointMatch(const size_t &idx) {
    note(5, (long)mnId, (long)idx, 0);
    mvpMapPoints[idx] = static_cast<MapPoint *>(NULL);
}
inline void KeyFrame::ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) {
    note(6, (long)mnId, (long)idx, (long)pMP->mnId);
    mvpMapPoints[idx] = pMP;
}
inline void Map::EraseMapPoint(MapPoint *pMP) {
    note(4, (long)pMP->mnId, 0, 0);
    mspMapPoints.erase(pMP);
}

}  // namespace fuse_standins
