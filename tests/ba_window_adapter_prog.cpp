// ba_window_adapter_prog.cpp — the two gathers of SIVO::LocalBundleAdjustment (sivo_amd/api/orbslam/OptimizerAdapter.h) on stand-in SLAM
// types over the host build of the C ABI (ba_window_host_capi.hpp), as a stand-alone program: `ba_window_adapter_prog gather IN OUT`
// builds TWO object graphs from one blob, runs optimizer_detail::gather_local_ba(pKF) — the walk — on the first and
// gather_local_ba(LocalMapDevice &, pKF) — LocalMapDevice::Rebuild, then ONE sivo_localmap_ba_window — on the second, and writes both
// LocalBAProblems.  tests/test_ba_window_host.py asks for equal bytes, plain and under the sanitizers.
//
//   in : tables (localmap_prog.cpp), i32 pKF, i32 mode (0; 1: the window is asked for a keyframe made after Rebuild; 2: such a keyframe is
//        the last covisible of pKF), arrays (i64 n + values) i32: cand (pKF, then its GetVectorCovisibleKeyFrames() in full), obs_idx
//        (mObservations' idx of every entry of obs_kf)
//   out: i32 status (1: an exception, then i32 length + its text, and nothing more), i64 sivo_localmap_ba_window calls made, then for the
//        walk and for the device gather alike: i64 length + the problem (problem()), and mnBALocalForKF of every keyframe and point and
//        mnBAFixedForKF of every keyframe as i64
// `ba_window_adapter_prog time REPS IN OUT` (tools/ba_window_probe.py) reads the same blob and writes f64 x 3, the median microseconds
// over REPS runs of the walk, of the device gather over the host build, and of that gather without the time inside
// sivo_localmap_ba_window (what the adapter does around the call), then i64 x 4: keyframes, points, fixed keyframes and edges of the
// problem.  pKF gets a new mnId for every run, as every new keyframe has: the stamps of the run before mean nothing to it.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <exception>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "localmap_delta_host_capi.hpp"
#include "ba_window_host_capi.hpp"
#include "localmap_standins.hpp"

#include "OptimizerAdapter.h"

namespace standin_ba {

class KeyFrame;

class MapPoint {
 public:
    long unsigned int mnId = 0, mnBALocalForKF = 0;
    std::map<KeyFrame *, size_t> mObservations;
    bool mbBad = false;
    cv::Mat mWorldPos;
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    int GetIndexInKeyFrame(KeyFrame *pKF) {
        const auto it = mObservations.find(pKF);
        return it == mObservations.end() ? -1 : (int)it->second;
    }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    bool isBad() { return mbBad; }
    void SetWorldPos(const cv::Mat &X) { mWorldPos = X.clone(); }      // (these three: what the solve's write-back calls)
    void UpdateNormalAndDepth() {}
    void EraseObservation(KeyFrame *pKF) { mObservations.erase(pKF); }
};

class KeyFrame {
 public:
    long unsigned int mnId = 0, mnBALocalForKF = 0, mnBAFixedForKF = 0;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::set<KeyFrame *> mspChildren;
    KeyFrame *mpParent = nullptr;
    bool mbBad = false;
    cv::Mat Tcw;
    std::vector<cv::KeyPoint> mvKeysSemantic;
    std::vector<float> mvRight, mvInvLevelSigma2;
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::set<KeyFrame *> GetChildren() { return mspChildren; }
    KeyFrame *GetParent() { return mpParent; }
    cv::Mat GetPose() { return Tcw.clone(); }
    bool isBad() { return mbBad; }
    float fx = 500.f, fy = 500.f, cx = 320.f, cy = 240.f, mbf = 40.f;  // (from here on: what the solve and its write-back touch)
    void SetPose(const cv::Mat &T) { Tcw = T.clone(); }
    void SetCovariance(const double *) {}
    void EraseMapPointMatch(MapPoint *pMP) {
        for (MapPoint *&q : mvpMapPoints)
            if (q == pMP) q = nullptr;
    }
};

struct Map {
    std::mutex mMutexMapUpdate;
};

// The graph of a set of tables, the keyframes in one array in the tables' kf_order (so std::less<KeyFrame *> walks them in that order);
// poses, positions and keypoints are functions of the indices, every key of a keyframe different from its neighbours.
struct Graph {
    std::vector<KeyFrame> kfStore;
    std::vector<MapPoint> pointStore;
    std::vector<KeyFrame *> kf;
    std::vector<MapPoint *> point;

    Graph(const SivoLocalMapTables &t, const std::vector<int32_t> &obsIdx, int32_t pkf, const std::vector<int32_t> &cand)
        : kfStore((size_t)t.n_kf), pointStore((size_t)t.n_points), kf((size_t)t.n_kf), point((size_t)t.n_points) {
        const size_t K = (size_t)t.n_kf, P = (size_t)t.n_points;
        std::vector<size_t> keys(K, 1);
        for (size_t i = 0; i < K; ++i) kf[(size_t)(t.kf_order ? t.kf_order[i] : (int32_t)i)] = &kfStore[i];
        for (size_t k = 0; k < K; ++k) keys[k] = std::max<size_t>(1, (size_t)(t.slot_off[k + 1] - t.slot_off[k]));
        for (size_t p = 0; p < P; ++p) {
            point[p] = &pointStore[p];
            point[p]->mnId = p;
            point[p]->mbBad = t.point_bad[p] != 0;
            point[p]->mWorldPos = cv::Mat(3, 1, CV_32F);
            for (int r = 0; r < 3; ++r) point[p]->mWorldPos.at<float>(r, 0) = 0.25f * (float)((p * (size_t)(r + 3)) % 17) + (r == 2 ? 5.f : -2.f);
            for (int64_t o = t.obs_off[p]; o < t.obs_off[p + 1]; ++o) {
                const size_t k = (size_t)t.obs_kf[o], idx = (size_t)obsIdx[(size_t)o];
                point[p]->mObservations[kf[k]] = idx;
                keys[k] = std::max(keys[k], idx + 1);
            }
        }
        for (size_t k = 0; k < K; ++k) {
            KeyFrame *pKF = kf[k];
            pKF->mnId = k + 1;
            pKF->mbBad = t.kf_bad[k] != 0;
            for (int64_t s = t.slot_off[k]; s < t.slot_off[k + 1]; ++s) pKF->mvpMapPoints.push_back(t.slot_point[s] < 0 ? nullptr : point[(size_t)t.slot_point[s]]);
            for (int64_t c = t.covis_off[k]; c < t.covis_off[k + 1]; ++c) pKF->mvpOrderedConnectedKeyFrames.push_back(kf[(size_t)t.covis_kf[c]]);
            for (int64_t c = t.child_off[k]; c < t.child_off[k + 1]; ++c) pKF->mspChildren.insert(kf[(size_t)t.child_kf[c]]);
            if (t.parent[k] >= 0) pKF->mpParent = kf[(size_t)t.parent[k]];
            pKF->Tcw = cv::Mat::zeros(4, 4, CV_32F);
            for (int d = 0; d < 4; ++d) pKF->Tcw.at<float>(d, d) = 1.f;
            for (int r = 0; r < 3; ++r) pKF->Tcw.at<float>(r, 3) = 0.125f * (float)((k * (size_t)(r + 2)) % 9) - 0.5f;
            pKF->mvInvLevelSigma2 = {1.f, 0.694444f, 0.482253f, 0.334898f};
            for (size_t i = 0; i < keys[k]; ++i) {
                cv::KeyPoint kp;
                kp.pt.x = (float)((7 * k + 13 * i) % 640) + 0.5f;
                kp.pt.y = (float)((11 * k + 5 * i) % 480) + 0.25f;
                kp.octave = (int)((k + i) % 4);
                pKF->mvKeysSemantic.push_back(kp);
                pKF->mvRight.push_back((k + i) % 3 == 0 ? kp.pt.x - 3.f - (float)(i % 5) : -1.f);
            }
        }
        kf[(size_t)pkf]->mvpOrderedConnectedKeyFrames.clear();
        for (size_t i = 1; i < cand.size(); ++i) kf[(size_t)pkf]->mvpOrderedConnectedKeyFrames.push_back(kf[(size_t)cand[i]]);
    }
};

typedef SIVO::optimizer_detail::LocalBAProblem<KeyFrame, MapPoint> Problem;

// every field of the problem, the pointers as table indices, poseIndex in index order
void problem(BlobWriter &w, const Problem &P) {
    BlobWriter b;
    auto kfs = [&](const std::vector<KeyFrame *> &v) {
        std::vector<int32_t> out(1, (int32_t)v.size());
        for (KeyFrame *k : v) out.push_back((int32_t)k->mnId - 1);
        b.put(out);
    };
    auto points = [&](const std::vector<MapPoint *> &v) {
        std::vector<int32_t> out(1, (int32_t)v.size());
        for (MapPoint *p : v) out.push_back((int32_t)p->mnId);
        b.put(out);
    };
    kfs(P.localKFs); points(P.localPoints);
    std::map<int32_t, int32_t> byIndex;
    for (const auto &e : P.poseIndex) byIndex[(int32_t)e.first->mnId - 1] = (int32_t)e.second;
    std::vector<int32_t> pi(1, (int32_t)byIndex.size());
    for (const auto &e : byIndex) { pi.push_back(e.first); pi.push_back(e.second); }
    b.put(pi);
    b.put(P.poses); b.put(P.fixedPose); b.put(P.points);
    const int64_t nE = (int64_t)P.edges.size();
    b.put(&nE, 1);
    b.put(P.edges);
    kfs(P.edgeKF); points(P.edgeMP);
    const int64_t n = (int64_t)b.buf.size();
    w.put(&n, 1);
    w.put(b.buf);
}

void stamps(BlobWriter &w, const Graph &g) {
    std::vector<int64_t> s;
    for (KeyFrame *k : g.kf) s.push_back((int64_t)k->mnBALocalForKF);
    for (MapPoint *p : g.point) s.push_back((int64_t)p->mnBALocalForKF);
    for (KeyFrame *k : g.kf) s.push_back((int64_t)k->mnBAFixedForKF);
    w.put(s);
}

}  // namespace standin_ba

#ifdef BA_WINDOW_WHOLE_CALL
// Compiled only by the syntax check of tests/test_ba_window_host.py (the solve needs the library and a device): the public overload
// SIVO::LocalBundleAdjustment(LocalMapDevice &, pKF, pbStopFlag, pMap) instantiated on the stand-in types.
void whole_call(SIVO::LocalMapDevice<standin_ba::KeyFrame, standin_ba::MapPoint> &dev, standin_ba::KeyFrame *pKF, bool *pbStopFlag, standin_ba::Map *pMap) {
    SIVO::LocalBundleAdjustment(dev, pKF, pbStopFlag, pMap);
    SIVO::LocalBundleAdjustment(pKF, pbStopFlag, pMap);
}
#endif

namespace {

double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int time_gathers(int reps, const char *in, const char *out) {
    using namespace standin_ba;
    typedef std::chrono::steady_clock Clock;
    BlobReader r(in);
    const LmBlobTables T(r);
    const SivoLocalMapTables t = T.table();
    const int32_t pkf = r.one<int32_t>();
    (void)r.one<int32_t>();
    const LmArr<int32_t> cand(r), obsIdx(r);
    Graph g(t, obsIdx.v, pkf, cand.v);
    KeyFrame *pKF = g.kf[(size_t)pkf];
    SIVO::LocalMapDevice<KeyFrame, MapPoint> dev;
    dev.Rebuild(g.kf);
    std::vector<double> walk, gather, around;
    int64_t sizes[4] = {0, 0, 0, 0};
    for (int i = 0; i < std::max(reps, 1); ++i) {
        pKF->mnId += (size_t)t.n_kf;
        auto t0 = Clock::now();
        const Problem a = SIVO::optimizer_detail::gather_local_ba(pKF);
        walk.push_back(std::chrono::duration<double, std::micro>(Clock::now() - t0).count());
        pKF->mnId += (size_t)t.n_kf;
        const double inside = ba_window_host::seconds();
        t0 = Clock::now();
        const Problem b = SIVO::optimizer_detail::gather_local_ba(dev, pKF);
        gather.push_back(std::chrono::duration<double, std::micro>(Clock::now() - t0).count());
        around.push_back(gather.back() - 1e6 * (ba_window_host::seconds() - inside));
        if (a.edges.size() != b.edges.size() || a.poses != b.poses || a.points != b.points) throw std::runtime_error("the two gathers differ");
        sizes[0] = (int64_t)a.localKFs.size(); sizes[1] = (int64_t)a.localPoints.size();
        sizes[2] = (int64_t)a.fixedPose.size() - sizes[0]; sizes[3] = (int64_t)a.edges.size();
    }
    const double res[3] = {median(walk), median(gather), median(around)};
    BlobWriter w;
    w.put(res, 3); w.put(sizes, 4);
    w.save(out);
    return 0;
}

int run(int argc, char **argv) {
    using namespace standin_ba;
    if (argc == 5 && std::string(argv[1]) == "time") return time_gathers(std::atoi(argv[2]), argv[3], argv[4]);
    if (argc != 4 || std::string(argv[1]) != "gather") throw BlobUsage();
    BlobReader r(argv[2]);
    BlobWriter w;
    const LmBlobTables T(r);
    const SivoLocalMapTables t = T.table();
    const int32_t pkf = r.one<int32_t>(), mode = r.one<int32_t>();
    const LmArr<int32_t> cand(r), obsIdx(r);
    Graph walk(t, obsIdx.v, pkf, cand.v), resident(t, obsIdx.v, pkf, cand.v);
    KeyFrame late;
    late.mnId = (size_t)t.n_kf + 1;
    int32_t status = 0;
    try {
        const Problem a = SIVO::optimizer_detail::gather_local_ba(walk.kf[(size_t)pkf]);
        SIVO::LocalMapDevice<KeyFrame, MapPoint> dev;
        dev.Rebuild(resident.kf);
        if (mode == 2) resident.kf[(size_t)pkf]->mvpOrderedConnectedKeyFrames.push_back(&late);
        const Problem b = SIVO::optimizer_detail::gather_local_ba(dev, mode == 1 ? &late : resident.kf[(size_t)pkf]);
        const int64_t calls = ba_window_host::calls();
        w.put(&status, 1); w.put(&calls, 1);
        problem(w, a); stamps(w, walk);
        problem(w, b); stamps(w, resident);
    } catch (const std::exception &e) {
        status = 1;
        const std::string msg = e.what();
        const int32_t n = (int32_t)msg.size();
        w.buf.clear();
        w.put(&status, 1); w.put(&n, 1); w.put(msg.data(), msg.size());
    }
    w.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "ba_window_adapter_prog gather IN OUT | time REPS IN OUT", run); }
