// Forced include (-include) of the oracle/_ref build of the reference's loop closer: LoopClosing.cc, KeyFrame.cc, MapPoint.cc, Map.cc and
// Converter.cc, compiled untouched with their own headers LoopClosing.h / KeyFrame.h / MapPoint.h / Map.h / Converter.h, so those classes are
// the reference's, member for member.  What ref_shims_mapgraph/mapgraph_standins.h provides is reused as it is (Frame, ORBextractor,
// ORBVocabulary, KeyFrameDatabase, System, the viewers, PnPsolver, cv::FileStorage); REF_LOOPCLOSING_BUILD takes its LoopClosing, Converter,
// Optimizer and ORBmatcher holders out.  Declared here instead, under the reference's names and with its signatures:
//   * LocalMapping, Tracking, Sim3Solver: data holders.  LocalMapping::RequestStop sets stopped, so the waits of LoopClosing.cc:427 / :686
//     end at once;
//   * Optimizer: OptimizeEssentialGraph hands its arguments to the driver's hook (the snapshot point of CorrectLoop, :582);
//     GlobalBundleAdjustment does nothing but set *pbStopFlag where the driver asks for it; OptimizeSim3 is linked only;
//   * ORBmatcher: DescriptorDistance is a popcount (the reference's own is pinned by tests/test_pin_matcher.py).  Fuse(pKF, Scw, points, th,
//     replace) is SCRIPTED: the driver names, per keyframe, which loop point lands on which slot; what follows from there is stated from
//     ORBmatcher.cc:962-963 / :1040-1047 (a bad point or one pKF already holds is passed over; a slot that holds a good point is reported
//     for replacement, an empty one takes the point and the observation).  The candidate choice of the real Fuse is therefore NOT part of
//     this build; the order of the calls, the graph each call meets, the deferred Replace calls and MapPoint::Replace /
//     ComputeDistinctiveDescriptors themselves are the reference's.  Every call is recorded;
//   * g2o::Sim3, Eigen::Quaterniond: ref_shims_loopclosing/g2o_sim3_standin.hpp (see there).
// Test infrastructure only.
#pragma once
#define REF_LOOPCLOSING_BUILD
#define LOCALMAPPING_H
#define TRACKING_H
#define SIM3SOLVER_H
#include "../ref_shims_mapgraph/mapgraph_standins.h"
#include "g2o_sim3_standin.hpp"

#include <functional>

namespace SIVO {

class LocalMapping {
 public:
    bool stopped = false, finished = false;
    int n_request_stop = 0, n_release = 0;
    void RequestStop() { stopped = true; ++n_request_stop; }
    bool isStopped() { return stopped; }
    bool isFinished() { return finished; }
    void Release() { stopped = false; ++n_release; }
};
class Tracking {};

class Sim3Solver {
 public:
    Sim3Solver(KeyFrame *, KeyFrame *, const std::vector<MapPoint *> &, const bool = true) {}
    void SetRansacParameters(double = 0.99, int = 6, int = 300) {}
    cv::Mat iterate(int, bool &bNoMore, std::vector<bool> &, int &nInliers) { bNoMore = true; nInliers = 0; return cv::Mat(); }
    cv::Mat GetEstimatedRotation() { return cv::Mat(); }
    cv::Mat GetEstimatedTranslation() { return cv::Mat(); }
    float GetEstimatedScale() { return 1.f; }
};

// what the stand-in matcher is told and what it met (one per process: the driver runs one scene per process)
struct FuseScript {
    struct Landing { int loop_point, slot; };
    struct Call {
        KeyFrame *kf;
        float scw[16];
        std::vector<int> action;                  // per landing of kf: 0 point bad, 1 already held, 2 replacement reported, 3 added, 4 slot holds a bad point
        std::vector<unsigned char> descriptor;    // per landing: the loop point's descriptor as the call met it (32 bytes; zeros where none)
    };
    std::map<KeyFrame *, std::vector<Landing> > landings;
    std::vector<Call> calls;
    static FuseScript &get() { static FuseScript s; return s; }
};

class ORBmatcher {
 public:
    ORBmatcher(float = 0.6, bool = true) {}
    static int DescriptorDistance(const cv::Mat &a, const cv::Mat &b) {
        int d = 0;
        for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a.ptr<unsigned char>()[i] ^ b.ptr<unsigned char>()[i]));
        return d;
    }
    int SearchByBoW(KeyFrame *, KeyFrame *, std::vector<MapPoint *> &) { return 0; }
    int SearchBySim3(KeyFrame *, KeyFrame *, std::vector<MapPoint *> &, const float &, const cv::Mat &, const cv::Mat &, const float) { return 0; }
    int SearchByProjection(KeyFrame *, cv::Mat, const std::vector<MapPoint *> &, std::vector<MapPoint *> &, int) { return 0; }
    inline int Fuse(KeyFrame *pKF, cv::Mat Scw, const std::vector<MapPoint *> &vpPoints, float th, std::vector<MapPoint *> &vpReplacePoint);
};

}  // namespace SIVO

// the reference's own classes, where they lie
#include "include/orbslam/LoopClosing.h"

namespace SIVO {

inline int ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, const std::vector<MapPoint *> &vpPoints, float, std::vector<MapPoint *> &vpReplacePoint) {
    FuseScript &s = FuseScript::get();
    FuseScript::Call rec;
    rec.kf = pKF;
    for (int i = 0; i < 16; ++i) rec.scw[i] = Scw.at<float>(i / 4, i % 4);
    const std::set<MapPoint *> spAlreadyFound = pKF->GetMapPoints();                  // ORBmatcher.cc:951
    int nFused = 0;
    for (const FuseScript::Landing &l : s.landings[pKF]) {
        MapPoint *pMP = vpPoints.at((size_t)l.loop_point);
        const cv::Mat d = pMP->GetDescriptor();
        for (int i = 0; i < 32; ++i) rec.descriptor.push_back(d.empty() ? 0 : d.ptr<unsigned char>()[i]);
        if (pMP->isBad()) { rec.action.push_back(0); continue; }                      // :962
        if (spAlreadyFound.count(pMP)) { rec.action.push_back(1); continue; }
        MapPoint *pMPinKF = pKF->GetMapPoint((size_t)l.slot);                         // :1040
        if (pMPinKF) {
            if (!pMPinKF->isBad()) { vpReplacePoint[(size_t)l.loop_point] = pMPinKF; rec.action.push_back(2); }
            else rec.action.push_back(4);
        } else {
            pMP->AddObservation(pKF, (size_t)l.slot);
            pKF->AddMapPoint(pMP, (size_t)l.slot);
            rec.action.push_back(3);
        }
        nFused++;
    }
    s.calls.push_back(rec);
    return nFused;
}

class Optimizer {
 public:
    typedef std::function<void(const LoopClosing::KeyFrameAndPose &NonCorrectedSim3, const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                               const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections)> Hook;
    static Hook &on_essential_graph() { static Hook h; return h; }
    static bool &stop_global_ba() { static bool b = false; return b; }
    static int &global_ba_calls() { static int n = 0; return n; }
    static void OptimizeEssentialGraph(Map *, KeyFrame *, KeyFrame *, const LoopClosing::KeyFrameAndPose &NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose &CorrectedSim3,
                                       const std::map<KeyFrame *, std::set<KeyFrame *> > &LoopConnections, const bool &) {
        if (on_essential_graph()) on_essential_graph()(NonCorrectedSim3, CorrectedSim3, LoopConnections);
    }
    static void GlobalBundleAdjustment(Map *, int = 5, bool *pbStopFlag = nullptr, const unsigned long = 0, const bool = true) {
        ++global_ba_calls();
        if (stop_global_ba() && pbStopFlag) *pbStopFlag = true;
    }
    static int OptimizeSim3(KeyFrame *, KeyFrame *, std::vector<MapPoint *> &, g2o::Sim3 &, const float, const bool) { return 0; }
};

}  // namespace SIVO
