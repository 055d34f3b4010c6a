// Forced include (-include) of the oracle/_ref builds of the reference's PnPsolver.cc and Sim3Solver.cc.  Their own headers
// PnPsolver.h / Sim3Solver.h are read where they lie, so the classes have the reference's members and layout; the headers those
// include for the SLAM graph (MapPoint.h, Frame.h, KeyFrame.h, ORBmatcher.h: Caffe, DBoW2's vocabulary, Eigen, threads) are
// switched off through their include guards and replaced by the data holders below, with the reference's member names.
#pragma once
#define MAPPOINT_H
#define FRAME_H
#define KEYFRAME_H
#define ORBMATCHER_H
#define EIGEN_MAKE_ALIGNED_OPERATOR_NEW

#include <algorithm>
#include <cmath>
#include <vector>
#include <opencv2/core/core.hpp>

using namespace std;      // (the reference's headers rely on one of the headers replaced here for it)

namespace SIVO {

class KeyFrame;

class MapPoint {
 public:
    cv::Mat mWorldPos = cv::Mat(3, 1, CV_32F);
    bool mbBad = false;
    KeyFrame *mpKF[2] = {nullptr, nullptr};      // the two keyframes of a Sim3 candidate and the point's index in each
    int mnIndex[2] = {-1, -1};
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool isBad() { return mbBad; }
    int GetIndexInKeyFrame(KeyFrame *pKF) { return pKF == mpKF[0] ? mnIndex[0] : pKF == mpKF[1] ? mnIndex[1] : -1; }
};

class Frame {
 public:
    float fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<cv::KeyPoint> mvKeysSemantic;
    std::vector<float> mvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
};

class KeyFrame {
 public:
    cv::Mat mK = cv::Mat(cv::Mat::zeros(3, 3, CV_32F));
    cv::Mat Tcw = cv::Mat(cv::Mat::eye(4, 4, CV_32F));
    std::vector<cv::KeyPoint> mvKeysSemantic;
    std::vector<float> mvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
    cv::Mat GetTranslation() { return Tcw.rowRange(0, 3).col(3).clone(); }
};

}  // namespace SIVO
