// Test program of tests/test_essential_graph_host.py and tests/test_gpu_essential_graph.py: Optimizer::OptimizeEssentialGraph (and its
// gather and write-back steps) over minimal KeyFrame / MapPoint / Map / Sim3 stand-ins.  Reads a map in the text form of
// essential_graph_restatement.map_text on stdin, prints hex floats.
//   gather: the vertices (id, vertex, fixed, siw) and the edges (i, j, meas) optimizer_detail::gather_essential_graph builds
//   pose:   optimizer_detail::cv_pose_from_sim3 of every line of 8 doubles after the map (the write-back of one keyframe)
//   run:    (-DSIVO_ESSENTIAL_GRAPH_ON_DEVICE, linked against libsivo_hip.so) every keyframe's pose and every map point's position after
//           Optimizer::OptimizeEssentialGraph
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "orbslam/Optimizer.h"

struct TKeyFrame;
struct TMapPoint {
    cv::Mat pos = cv::Mat(3, 1, CV_32F);
    bool bad = false;
    unsigned long mnCorrectedByKF = 0, mnCorrectedReference = 0;
    TKeyFrame *ref = nullptr;
    cv::Mat GetWorldPos() const { return pos.clone(); }
    void SetWorldPos(const cv::Mat &X) { pos = X.clone(); }
    bool isBad() const { return bad; }
    TKeyFrame *GetReferenceKeyFrame() const { return ref; }
    void UpdateNormalAndDepth() {}
};
struct TKeyFrame {
    unsigned long mnId = 0;
    bool bad = false;
    cv::Mat Tcw = cv::Mat::eye(4, 4, CV_32F);
    TKeyFrame *parent = nullptr;
    std::set<TKeyFrame *> children, loops;
    std::vector<std::pair<TKeyFrame *, int>> ordered;          // connections by weight, descending
    bool isBad() const { return bad; }
    cv::Mat GetRotation() const { cv::Mat R(3, 3, CV_32F); for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R.at<float>(r, c) = Tcw.at<float>(r, c); return R; }
    cv::Mat GetTranslation() const { cv::Mat t(3, 1, CV_32F); for (int r = 0; r < 3; ++r) t.at<float>(r, 0) = Tcw.at<float>(r, 3); return t; }
    void SetPose(const cv::Mat &T) { Tcw = T.clone(); }
    TKeyFrame *GetParent() const { return parent; }
    bool hasChild(TKeyFrame *k) const { return children.count(k) != 0; }
    std::set<TKeyFrame *> GetLoopEdges() const { return loops; }
    int GetWeight(TKeyFrame *k) const { for (auto &c : ordered) if (c.first == k) return c.second; return 0; }
    // KeyFrame::GetCovisiblesByWeight (KeyFrame.cc:232-250), its upper_bound test included: nothing when every weight is >= w
    std::vector<TKeyFrame *> GetCovisiblesByWeight(int w) const {
        size_t n = 0;
        while (n < ordered.size() && ordered[n].second >= w) ++n;
        std::vector<TKeyFrame *> out;
        if (n == ordered.size()) return out;
        for (size_t i = 0; i < n; ++i) out.push_back(ordered[i].first);
        return out;
    }
};
struct TMap {
    std::vector<TKeyFrame *> kfs;
    std::vector<TMapPoint *> mps;
    unsigned long max_id = 0;
    std::mutex mMutexMapUpdate;
    std::vector<TKeyFrame *> GetAllKeyFrames() const { return kfs; }
    std::vector<TMapPoint *> GetAllMapPoints() const { return mps; }
    unsigned long GetMaxKFid() const { return max_id; }
};
struct TQuat {                         // Eigen::Quaterniond as g2o::Sim3::rotation() hands it out
    double c[4] = {0, 0, 0, 1};
    double &x() { return c[0]; } double &y() { return c[1]; } double &z() { return c[2]; } double &w() { return c[3]; }
    double x() const { return c[0]; } double y() const { return c[1]; } double z() const { return c[2]; } double w() const { return c[3]; }
};
struct TVec3 {
    double c[3] = {0, 0, 0};
    double &operator[](int i) { return c[i]; }
    double operator[](int i) const { return c[i]; }
};
struct TSim3 {
    TQuat r; TVec3 t; double s = 1;
    const TQuat &rotation() const { return r; }
    const TVec3 &translation() const { return t; }
    double scale() const { return s; }
};

static double rd() { double v; if (std::scanf("%lf", &v) != 1) std::exit(2); return v; }
static long ri() { return (long)rd(); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    const long nkf = ri(), npts = ri(), cur = ri(), loop = ri(), fix_scale = ri();
    std::vector<TKeyFrame> kf((size_t)nkf);
    std::vector<TMapPoint> mp((size_t)npts);
    TMap map;
    for (long k = 0; k < nkf; ++k) map.kfs.push_back(&kf[(size_t)ri()]);
    for (long k = 0; k < nkf; ++k) {
        TKeyFrame &K = kf[(size_t)k];
        K.mnId = (unsigned long)ri();
        K.bad = ri() != 0;
        const long par = ri();
        K.parent = par >= 0 ? &kf[(size_t)par] : nullptr;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) K.Tcw.at<float>(r, c) = (float)rd();
        for (long q = ri(); q > 0; --q) K.children.insert(&kf[(size_t)ri()]);
        for (long q = ri(); q > 0; --q) K.loops.insert(&kf[(size_t)ri()]);
        for (long q = ri(); q > 0; --q) { const long c = ri(); const int w = (int)ri(); K.ordered.push_back({&kf[(size_t)c], w}); }
        map.max_id = std::max(map.max_id, K.mnId);
    }
    std::map<TKeyFrame *, TSim3> poses[2];             // CorrectedSim3, NonCorrectedSim3
    for (auto &P : poses)
        for (long q = ri(); q > 0; --q) {
            TSim3 S;
            TKeyFrame *k = &kf[(size_t)ri()];
            for (int i = 0; i < 4; ++i) S.r.c[i] = rd();
            for (int i = 0; i < 3; ++i) S.t.c[i] = rd();
            S.s = rd();
            P[k] = S;
        }
    std::map<TKeyFrame *, std::set<TKeyFrame *>> conns;
    for (long q = ri(); q > 0; --q) {
        TKeyFrame *a = &kf[(size_t)ri()];
        for (long m = ri(); m > 0; --m) conns[a].insert(&kf[(size_t)ri()]);
    }
    for (TMapPoint &p : mp) {
        for (int r = 0; r < 3; ++r) p.pos.at<float>(r, 0) = (float)rd();
        p.bad = ri() != 0;
        p.ref = &kf[(size_t)ri()];
        p.mnCorrectedByKF = (unsigned long)ri();
        p.mnCorrectedReference = (unsigned long)ri();
        map.mps.push_back(&p);
    }
    TKeyFrame *pCur = &kf[(size_t)cur], *pLoop = &kf[(size_t)loop];
    if (mode == "gather") {
        std::vector<double> siw;
        std::vector<uint8_t> fixed, vertex;
        std::vector<SivoSim3Edge> edges;
        SIVO::optimizer_detail::gather_essential_graph(&map, pLoop, pCur, poses[1], poses[0], conns, siw, fixed, vertex, edges);
        std::printf("%zu %zu\n", fixed.size(), edges.size());
        for (size_t v = 0; v < fixed.size(); ++v) {
            std::printf("%d %d", (int)vertex[v], (int)fixed[v]);
            for (int i = 0; i < 8; ++i) std::printf(" %a", siw[8 * v + i]);
            std::printf("\n");
        }
        for (const SivoSim3Edge &e : edges) {
            std::printf("%d %d", e.i, e.j);
            for (int i = 0; i < 8; ++i) std::printf(" %a", e.meas[i]);
            std::printf("\n");
        }
        return 0;
    }
    if (mode == "pose") {
        double S[8];
        while (std::scanf("%lf", &S[0]) == 1) {
            for (int i = 1; i < 8; ++i) S[i] = rd();
            const cv::Mat T = SIVO::optimizer_detail::cv_pose_from_sim3(S);
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) std::printf("%a ", (double)T.at<float>(r, c));
            std::printf("\n");
        }
        return 0;
    }
#ifdef SIVO_ESSENTIAL_GRAPH_ON_DEVICE
    if (mode == "run") {
        SIVO::Optimizer::OptimizeEssentialGraph(&map, pLoop, pCur, poses[1], poses[0], conns, fix_scale != 0);
        for (const TKeyFrame &K : kf) {
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) std::printf("%a ", (double)K.Tcw.at<float>(r, c));
            std::printf("\n");
        }
        for (const TMapPoint &p : mp) std::printf("%a %a %a\n", (double)p.pos.at<float>(0, 0), (double)p.pos.at<float>(1, 0), (double)p.pos.at<float>(2, 0));
        return 0;
    }
#endif
    (void)fix_scale;
    return 2;
}
