// Forced include (-include) of the oracle/_ref builds of the reference's LocalMapping.cc and MapPoint.cc.  Their own headers
// LocalMapping.h / MapPoint.h are read where they lie, so the two classes have the reference's members; sivo_helpers.hpp is the
// reference's too (over ref_shims_eigen).  The headers those include for the rest of the system (KeyFrame.h, Frame.h, Map.h,
// LoopClosing.h, Tracking.h, KeyFrameDatabase.h, ORBmatcher.h, Optimizer.h, bayesian_segnet.hpp: Caffe, DBoW2, g2o, threads) are switched
// off through their include guards and replaced by the data holders below, under the reference's member names and with its types.
// What the holders do themselves is trivial, with three exceptions that oracle/ref_localmapping_driver.cpp scripts or reads:
//   * ORBmatcher::SearchForTriangulation returns the match list the driver queued for that neighbour and records the F12 it was handed
//     and which slots of the current keyframe held a point at the call; ORBmatcher::Fuse records its calls;
//   * ORBmatcher::DescriptorDistance is a popcount (the reference's own is pinned by tests/test_pin_matcher.py);
//   * KeyFrame::UnprojectStereo is stated from the rules of cv_min.hpp (KeyFrame.cc is not compiled): a substitution, DESIGN.md §5.
#pragma once
#define KEYFRAME_H
#define FRAME_H
#define MAP_H
#define LOOPCLOSING_H
#define TRACKING_H
#define KEYFRAMEDATABASE_H
#define ORBMATCHER_H
#define OPTIMIZER_H
#define BAYESIAN_SEGNET_BAYESIAN_SEGNET_HPP
#ifndef EIGEN_MAKE_ALIGNED_OPERATOR_NEW
#define EIGEN_MAKE_ALIGNED_OPERATOR_NEW
#endif

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include <opencv2/core/core.hpp>

#include "sivo_helpers/sivo_helpers.hpp"

using namespace std;      // (the reference's sources rely on one of the headers replaced here for it)

namespace SIVO {

// the label ids of the network's output, in its order; VOID is what a rejected keypoint carries
enum Classes { ROAD, SIDEWALK, BUILDING, WALL, POLE, TRAFFIC_LIGHT, TRAFFIC_SIGN, VEGETATION, TERRAIN, SKY, PERSON, CAR, COMMERCIAL_VEHICLE, BIKE, VOID = 255 };

class MapPoint;
class KeyFrame;

// mEntropy / mConfidence / mClasses (row, col): only the pixels the driver painted; `conflict` is set when a pixel is painted twice
// with different values
template <class T>
struct PixelMap {
    std::map<std::pair<int, int>, T> v;
    bool conflict = false;
    void paint(int row, int col, T value) {
        auto it = v.find(std::make_pair(row, col));
        if (it == v.end()) v[std::make_pair(row, col)] = value;
        else if (!(it->second == value)) conflict = true;
    }
    T operator()(int row, int col) const { auto it = v.find(std::make_pair(row, col)); return it == v.end() ? T() : it->second; }
};

class Frame {
 public:
    long unsigned int mnId = 0;
    int mnScaleLevels = 0;
    float mfLogScaleFactor = 0;
    std::vector<cv::KeyPoint> mvKeysSemantic;
    std::vector<float> mvScaleFactors;
    cv::Mat mDescriptorsSemantic, mOw = cv::Mat(cv::Mat::zeros(3, 1, CV_32F));
    cv::Mat GetCameraCenter() { return mOw.clone(); }
};

class KeyFrame {
 public:
    long unsigned int mnId = 0, mnFrameId = 0, mnFuseTargetForKF = 0;
    float fx = 1, fy = 1, cx = 0, cy = 0, invfx = 1, invfy = 1, mbf = 0, mb = 0, mThDepth = 0, mThConfidence = 0, mThEntropyReduction = 0;
    float mfScaleFactor = 1.2f, mfLogScaleFactor = 0;
    int mnScaleLevels = 0, numSemanticKeys = 0;
    std::vector<float> mvScaleFactors, mvLevelSigma2, mvRight, mvDepth;
    std::vector<cv::KeyPoint> mvKeysSemantic;
    cv::Mat mDescriptorsSemantic;
    cv::Mat mK = cv::Mat(cv::Mat::eye(3, 3, CV_32F)), mTcw = cv::Mat(cv::Mat::eye(4, 4, CV_32F)), mTwc = cv::Mat(cv::Mat::eye(4, 4, CV_32F));
    cv::Mat mOw = cv::Mat(cv::Mat::zeros(3, 1, CV_32F));
    PixelMap<double> mEntropy, mConfidence;
    PixelMap<int> mClasses;
    StateCovarianceType mSigma;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<KeyFrame *> ordered;                      // mvpOrderedConnectedKeyFrames
    bool mbBad = false;
    float medianDepth = 1;                                // what ComputeSceneMedianDepth returns (scripted)
    int nUpdateConnections = 0, nMedianDepthCalls = 0;

    cv::Mat GetRotation() { return mTcw.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation() { return mTcw.rowRange(0, 3).col(3).clone(); }
    cv::Mat GetCameraCenter() { return mOw.clone(); }
    StateCovarianceType GetCovariance() const { return mSigma; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N) {
        return (int)ordered.size() < N ? ordered : std::vector<KeyFrame *>(ordered.begin(), ordered.begin() + N);
    }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return ordered; }
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    MapPoint *GetMapPoint(const size_t &idx) { return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t &idx) { mvpMapPoints[idx] = nullptr; }
    void ReplaceMapPointMatch(const size_t &idx, MapPoint *pMP) { mvpMapPoints[idx] = pMP; }
    bool isBad() { return mbBad; }
    void SetBadFlag() { mbBad = true; }
    void ComputeBoW() {}
    void UpdateConnections() { ++nUpdateConnections; }
    float ComputeSceneMedianDepth(const int) { ++nMedianDepthCalls; return medianDepth; }
    // the keypoint's depth along its ray, taken to the world by the inverse pose as one product-and-add
    cv::Mat UnprojectStereo(const unsigned long i) {
        const float z = mvDepth[i];
        if (!(z > 0)) return cv::Mat();
        const float x = (mvKeysSemantic[i].pt.x - cx) * z * invfx, y = (mvKeysSemantic[i].pt.y - cy) * z * invfy;
        cv::Mat c(3, 1, CV_32F);
        c.at<float>(0) = x; c.at<float>(1) = y; c.at<float>(2) = z;
        return mTwc.rowRange(0, 3).colRange(0, 3) * c + mTwc.rowRange(0, 3).col(3);
    }
};

class Map {
 public:
    std::mutex mMutexPointCreation;
    std::vector<MapPoint *> added, erased;
    std::vector<KeyFrame *> keyframes;
    void AddKeyFrame(KeyFrame *pKF) { keyframes.push_back(pKF); }
    void AddMapPoint(MapPoint *pMP) { added.push_back(pMP); }
    void EraseMapPoint(MapPoint *pMP) { erased.push_back(pMP); }
    long unsigned KeyFramesInMap() { return keyframes.size(); }
};

class LoopClosing {
 public:
    std::vector<KeyFrame *> inserted;
    void InsertKeyFrame(KeyFrame *pKF) { inserted.push_back(pKF); }
};
class Tracking {};
class KeyFrameDatabase {};

class Optimizer {
 public:
    static void LocalBundleAdjustment(KeyFrame *, bool *, Map *) {}
};

// what the stand-in matcher was asked and what it answers (one per process: the driver runs one scene per process)
struct MatcherScript {
    std::map<KeyFrame *, std::vector<std::pair<size_t, size_t> > > matches;      // per neighbour
    struct Search { KeyFrame *kf2; float F12[9]; std::vector<uint8_t> occupied1; };
    std::vector<Search> searches;
    struct FuseCall { KeyFrame *kf; std::vector<MapPoint *> points; };
    std::vector<FuseCall> fuses;
    void (*on_search)(KeyFrame *kf2) = nullptr;      // the driver's hook, called first: it may queue the matches by what is free now
    static MatcherScript &get() { static MatcherScript s; return s; }
};

class ORBmatcher {
 public:
    ORBmatcher(float = 0.6, bool = true) {}
    int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, std::vector<std::pair<size_t, size_t> > &vMatchedPairs, const bool) {
        MatcherScript &s = MatcherScript::get();
        MatcherScript::Search rec;
        rec.kf2 = pKF2;
        for (int i = 0; i < 9; ++i) rec.F12[i] = F12.at<float>(i / 3, i % 3);
        for (MapPoint *p : pKF1->mvpMapPoints) rec.occupied1.push_back(p != nullptr);
        s.searches.push_back(rec);
        if (s.on_search) s.on_search(pKF2);
        vMatchedPairs = s.matches[pKF2];
        return (int)vMatchedPairs.size();
    }
    int Fuse(KeyFrame *pKF, const std::vector<MapPoint *> &vpMapPoints, const float = 3.0) {
        MatcherScript::get().fuses.push_back(MatcherScript::FuseCall{pKF, vpMapPoints});
        return 0;
    }
    static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b) {
        int d = 0;
        for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a.ptr<unsigned char>()[i] ^ b.ptr<unsigned char>()[i]));
        return d;
    }
};

}  // namespace SIVO

// KeyFrame.h is what hands MapPoint.h to LocalMapping.cc in the reference: the reference's own MapPoint.h, where it lies
#include "include/orbslam/MapPoint.h"
