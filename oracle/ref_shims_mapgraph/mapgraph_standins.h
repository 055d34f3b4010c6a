// Forced include (-include) of the oracle/_ref build of the reference's map graph: KeyFrame.cc, MapPoint.cc, Map.cc, LocalMapping.cc and
// Tracking.cc, compiled untouched with their own headers KeyFrame.h / MapPoint.h / Map.h / LocalMapping.h / Tracking.h, so the five classes
// are the reference's, member for member.  sivo_helpers.hpp is the reference's too (over ref_shims_eigen), and so are DBoW2's BowVector.h /
// FeatureVector.h.  Every other header those pull in (Frame.h, ORBextractor.h, ORBVocabulary.h, KeyFrameDatabase.h, LoopClosing.h, System.h,
// Viewer.h, FrameDrawer.h, MapDrawer.h, ORBmatcher.h, Optimizer.h, PnPsolver.h, Converter.h, bayesian_segnet.hpp: Caffe, DBoW2's vocabulary,
// g2o, Pangolin, the threads) is switched off through its include guard and replaced by the data holders below, under the reference's
// member names and with its types.  The holders do nothing of their own, with two exceptions oracle/ref_mapgraph_driver.cpp reads:
//   * KeyFrameDatabase::erase records its calls (KeyFrame::SetBadFlag calls it right after Map::EraseKeyFrame, KeyFrame.cc:566-567, so
//     the record is the order of the EraseKeyFrame calls as well; Map itself is the reference's class and keeps no order);
//   * cv::FileStorage answers a key with the number scripted for it.
// Test infrastructure only.
#pragma once
#define FRAME_H
#define ORBEXTRACTOR_H
#define ORBVOCABULARY_H
#define KEYFRAMEDATABASE_H
#ifndef REF_LOOPCLOSING_BUILD      // (ref_shims_loopclosing/loopclosing_standins.h: LoopClosing.h and Converter.h are the reference's there)
#define LOOPCLOSING_H
#define CONVERTER_H
#endif
#define SYSTEM_H
#define VIEWER_H
#define FRAMEDRAWER_H
#define MAPDRAWER_H
#define ORBMATCHER_H
#define OPTIMIZER_H
#define PNPSOLVER_H
#define BAYESIAN_SEGNET_BAYESIAN_SEGNET_HPP
#ifndef EIGEN_MAKE_ALIGNED_OPERATOR_NEW
#define EIGEN_MAKE_ALIGNED_OPERATOR_NEW
#endif
#define FRAME_GRID_ROWS 48
#define FRAME_GRID_COLS 64

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include <opencv2/core/core.hpp>

#include "sivo_helpers/sivo_helpers.hpp"
#include "dependencies/DBoW2/DBoW2/BowVector.h"
#include "dependencies/DBoW2/DBoW2/FeatureVector.h"

using namespace std;      // (the reference's sources rely on one of the headers replaced here for it)

namespace cv {
// the settings file: a key holds the number scripted for it, 1 where none is
struct FileNode {
    double v;
    operator float() const { return (float)v; }
    operator int() const { return (int)v; }
    operator double() const { return v; }
};
class FileStorage {
 public:
    enum { READ = 0 };
    static std::map<std::string, double> &scripted() { static std::map<std::string, double> v; return v; }
    FileStorage(const std::string &, int) {}
    FileNode operator[](const char *key) const {
        const auto it = scripted().find(key);
        return FileNode{it == scripted().end() ? 1.0 : it->second};
    }
};
// colour conversion of the input images: no image passes through this build
inline void cvtColor(const Mat &, Mat &, int) {}
// cv2eigen of the 4 x 4 float velocity (Tracking.cc:716)
inline void cv2eigen(const Mat &src, Eigen::Matrix4d &dst) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) dst(i, j) = src.at<float>(i, j);
}
}  // namespace cv
#define CV_RGB2GRAY 7
#define CV_BGR2GRAY 6
#define CV_RGBA2GRAY 11
#define CV_BGRA2GRAY 10

namespace SIVO {

// the label ids of the network's output, in its order; VOID is what a rejected keypoint carries
enum Classes { ROAD, SIDEWALK, BUILDING, WALL, POLE, TRAFFIC_LIGHT, TRAFFIC_SIGN, VEGETATION, TERRAIN, SKY, PERSON, CAR, COMMERCIAL_VEHICLE, BIKE, VOID = 255 };

// mEntropy / mConfidence / mClasses (row, col): empty here, every pixel reads as zero
template <class T>
struct PixelMap {
    std::map<std::pair<int, int>, T> v;
    T operator()(int row, int col) const { auto it = v.find(std::make_pair(row, col)); return it == v.end() ? T() : it->second; }
};
typedef PixelMap<int> MatXu;
typedef PixelMap<double> MatXd;

class MapPoint;
class KeyFrame;
class Map;
class Frame;
class Tracking;
class LocalMapping;

class BayesianSegNet {};
class ORBVocabulary {
 public:
    void transform(const std::vector<cv::Mat> &, DBoW2::BowVector &, DBoW2::FeatureVector &, int) {}
    double score(const DBoW2::BowVector &, const DBoW2::BowVector &) const { return 0; }
};
class ORBextractor {
 public:
    ORBextractor(int, float, int, int, int) {}
};
#ifndef REF_LOOPCLOSING_BUILD
struct Converter {
    static std::vector<cv::Mat> toDescriptorVector(const cv::Mat &) { return std::vector<cv::Mat>(); }
};
#endif

class Frame {
 public:
    Frame() {}
    Frame(const cv::Mat &, const cv::Mat &, const cv::Mat &, const double &timeStamp, ORBextractor *, ORBextractor *, ORBVocabulary *,
          BayesianSegNet *, cv::Mat &, cv::Mat &, const float &, const float &, const float &, const float &) : mTimeStamp(timeStamp) {}
    cv::Mat getSegmentedImage() { return mImSemantic; }
    void ComputeBoW() {}
    void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); }
    void SetCovariance(const StateCovarianceType &Sigmacw) { mSigmacw = Sigmacw; }
    void UpdatePoseMatrices() {}
    cv::Mat GetCameraCenter() { return mOw.clone(); }
    cv::Mat GetRotationInverse() { return mRwc.clone(); }
    bool isInFrustum(MapPoint *, float) { return false; }
    cv::Mat UnprojectStereo(const unsigned long &) { return cv::Mat(); }

    ORBVocabulary *mpORBvocabulary = nullptr;
    ORBextractor *mpORBextractorLeft = nullptr, *mpORBextractorRight = nullptr;
    BayesianSegNet *mpBayesianSegNet = nullptr;
    double mTimeStamp = 0;
    cv::Mat mK = cv::Mat(cv::Mat::eye(3, 3, CV_32F)), mDistCoef, mImSemantic;
    float fx = 1, fy = 1, cx = 0, cy = 0, invfx = 1, invfy = 1;
    float mbf = 0, mb = 0, mThDepth = 0, mThConfidence = 0, mThEntropyReduction = 0;
    int numSemanticKeys = 0;
    std::vector<cv::KeyPoint> mvKeysLeft, mvKeysSemantic, mvKeysRight;
    std::vector<float> mvRight, mvDepth;
    MatXu mClasses;
    MatXd mConfidence, mEntropy;
    DBoW2::BowVector mBowVec;
    DBoW2::FeatureVector mFeatVec;
    cv::Mat mDescriptorsLeft, mDescriptorsRight, mDescriptorsSemantic;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    float mfGridElementWidthInv = 1, mfGridElementHeightInv = 1;
    std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];
    cv::Mat mTcw = cv::Mat(cv::Mat::eye(4, 4, CV_32F));
    StateCovarianceType mSigmacw;
    static long unsigned int nNextId;                     // (defined in the driver)
    static bool mbInitialComputations;
    long unsigned int mnId = 0;
    KeyFrame *mpReferenceKF = nullptr;
    int mnScaleLevels = 1;
    float mfScaleFactor = 1.2f, mfLogScaleFactor = 0;
    std::vector<float> mvScaleFactors, mvInvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
    cv::Mat mRwc = cv::Mat(cv::Mat::eye(3, 3, CV_32F)), mOw = cv::Mat(cv::Mat::zeros(3, 1, CV_32F));
};

class KeyFrameDatabase {
 public:
    std::vector<KeyFrame *> erased;                       // the calls of erase, in order
    void add(KeyFrame *) {}
    void erase(KeyFrame *pKF) { erased.push_back(pKF); }
    void clear() {}
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *) { return std::vector<KeyFrame *>(); }
    std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame *, float) { return std::vector<KeyFrame *>(); }
};

#ifndef REF_LOOPCLOSING_BUILD
class LoopClosing {
 public:
    void InsertKeyFrame(KeyFrame *) {}
    void RequestReset() {}
};
#endif
class System {
 public:
    enum eSensor { MONOCULAR = 0, STEREO = 1, RGBD = 2 };
    void Reset() {}
};
class Viewer {
 public:
    void RequestStop() {}
    bool isStopped() { return true; }
    void Release() {}
};
class FrameDrawer {
 public:
    void Update(Tracking *) {}
};
class MapDrawer {
 public:
    void SetCurrentCameraPose(const cv::Mat &) {}
};

#ifndef REF_LOOPCLOSING_BUILD
class Optimizer {
 public:
    static void LocalBundleAdjustment(KeyFrame *, bool *, Map *) {}
    static int PoseOptimization(Frame *) { return 0; }
};

class ORBmatcher {
 public:
    ORBmatcher(float = 0.6, bool = true) {}
    int SearchForTriangulation(KeyFrame *, KeyFrame *, cv::Mat, std::vector<std::pair<size_t, size_t> > &, const bool) { return 0; }
    int Fuse(KeyFrame *, const std::vector<MapPoint *> &, const float = 3.0) { return 0; }
    int SearchByProjection(Frame &, const std::vector<MapPoint *> &, const float = 3) { return 0; }
    int SearchByProjection(Frame &, const Frame &, const float, const bool) { return 0; }
    int SearchByProjection(Frame &, KeyFrame *, const std::set<MapPoint *> &, const float, const int) { return 0; }
    int SearchByBoW(KeyFrame *, Frame &, std::vector<MapPoint *> &) { return 0; }
    static int DescriptorDistance(const cv::Mat &, const cv::Mat &) { return 0; }
};
#endif

class PnPsolver {
 public:
    PnPsolver(const Frame &, const std::vector<MapPoint *> &) {}
    void SetRansacParameters(double = 0.99, int = 8, int = 300, int = 4, float = 0.4, float = 5.991) {}
    cv::Mat iterate(int, bool &bNoMore, std::vector<bool> &, int &nInliers) { bNoMore = true; nInliers = 0; return cv::Mat(); }
};

}  // namespace SIVO
