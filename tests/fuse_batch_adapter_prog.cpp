// fuse_batch_adapter_prog.cpp — SIVO::FuseIntoKeyFrames and SIVO::SearchAndFuse (sivo_amd/api/orbslam/FusionAdapter.h) against the loops
// they replace — `for (pKFi : vpTargetKFs) matcher.Fuse(pKFi, vpMapPoints, th)` (reference LocalMapping.cc:586-594) and
// LoopClosing::SearchAndFuse (LoopClosing.cc:609-635) written out with this repository's single-keyframe ORBmatcher::Fuse members — on two
// copies of one object graph of stand-ins (fuse_batch_standins.hpp), as a stand-alone program: `fuse_batch_adapter_prog fuse|loop IN OUT`.
// By default the C ABI under both is the host build (fuse_batch_host_capi.hpp: no library, no device, fit for the sanitizers); with
// -DFUSE_BATCH_ON_LIBRARY the program links libsivo_hip instead and both sides run on the device.
//
// The keyframes of a graph live in one array, so that pointer order — which std::map / std::set follow — is the scene's order in both
// copies.  Every array in the blob is an i64 length followed by that many items (tests/fuse_batch_adapter_cases.py writes it):
//   i32 K, P, flags (bit 0: the adapter's repair step switched off), f32 th, intr f32[5] (fx fy cx cy bf), bounds i32[4], scale f32[levels],
//   log_scale f32[1]; per keyframe: bad u8[1], pose f32[12] (R row-major, t), ow f32[3], scw f32[16], x f32, y f32, octave i32, right f32,
//   desc u8, slot i32 (the map point in each slot, -1 none); pos f32[3 P], normal f32[3 P], min_dist f32[P], max_dist f32[P], desc u8[32 P],
//   bad u8[P], list i32 (indices into the points, -1 a null entry), targets i32 (the target keyframes in the loop's order; `loop`: ascending)
//   -> two dumps, the adapter's graph and the loop's: nFused i32[K], i64 events, events i64[4 each], per keyframe slot i32[n] (point id, -1
//      none), per point bad u8, nObs i32, found i32, visible i32, replaced-by i32, desc u8[32], i64 observations, (keyframe id, idx) i64
//      pairs; then i32 batch calls, single calls, repair calls of the adapter's run (zeros when linked against the library)
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "blob_io.hpp"
#ifndef FUSE_BATCH_ON_LIBRARY
#include "fuse_batch_host_capi.hpp"
#endif
#include "fuse_batch_standins.hpp"
#include "orbslam/FusionAdapter.h"

// (the program links neither sivo_amd/api's ORBmatcher.cc nor anything else of the class library: the one member it needs)
SIVO::ORBmatcher::ORBmatcher(float nnratio, bool checkOri) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

namespace {
using namespace fuse_standins;

template <class T> std::vector<T> arr(BlobReader &r, size_t want = (size_t)-1) {
    const int64_t n = r.one<int64_t>();
    if (n < 0 || (want != (size_t)-1 && (size_t)n != want)) throw std::runtime_error("an array of the scene has the wrong length");
    return r.many<T>((size_t)n);
}

struct SceneKf {
    uint8_t bad;
    std::vector<float> pose, ow, scw, x, y, right;
    std::vector<int32_t> oct, slot;
    std::vector<uint8_t> desc;
};
struct Scene {
    int32_t K, P, flags;
    float th;
    std::vector<float> intr, scale, log_scale, pos, normal, mn, mx;
    std::vector<int32_t> bounds, list, targets;
    std::vector<SceneKf> kf;
    std::vector<uint8_t> desc, bad;
};

struct Graph {
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> pts;
    Map map;
    std::vector<Event> log;
    std::vector<MapPoint *> list;
    std::vector<KeyFrame *> targets;
    std::map<KeyFrame *, cv::Mat> poses;
};

cv::Mat mat(const float *v, int rows, int cols) {
    cv::Mat M(rows, cols, CV_32F);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) M.at<float>(r, c) = v[cols * r + c];
    return M;
}

void build(const Scene &s, Graph &g) {
    g.kfs.resize((size_t)s.K);
    g.pts.resize((size_t)s.P);
    for (int32_t p = 0; p < s.P; ++p) {
        MapPoint &m = g.pts[(size_t)p];
        m.mnId = (long unsigned int)p;
        m.mWorldPos = mat(&s.pos[3 * (size_t)p], 3, 1);
        m.mNormalVector = mat(&s.normal[3 * (size_t)p], 3, 1);
        m.mfMinDistance = s.mn[(size_t)p]; m.mfMaxDistance = s.mx[(size_t)p];
        m.mDescriptor = cv::Mat(1, 32, CV_8U);
        std::memcpy(m.mDescriptor.ptr(0), &s.desc[32 * (size_t)p], 32);
        m.mbBad = s.bad[(size_t)p] != 0;
        m.mpMap = &g.map;
        if (!m.mbBad) g.map.mspMapPoints.insert(&m);
    }
    for (int32_t k = 0; k < s.K; ++k) {
        const SceneKf &in = s.kf[(size_t)k];
        KeyFrame &f = g.kfs[(size_t)k];
        const size_t n = in.x.size();
        f.mnId = (long unsigned int)(100 + k);
        f.mbBad = in.bad != 0;
        f.mvKeysSemantic.resize(n);
        for (size_t i = 0; i < n; ++i) { f.mvKeysSemantic[i].pt.x = in.x[i]; f.mvKeysSemantic[i].pt.y = in.y[i]; f.mvKeysSemantic[i].octave = in.oct[i]; }
        f.mvRight = in.right;
        f.mDescriptorsSemantic = cv::Mat((int)n, 32, CV_8U);
        if (n) std::memcpy(f.mDescriptorsSemantic.data, in.desc.data(), 32 * n);
        f.mTcw = cv::Mat::eye(4, 4, CV_32F);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) f.mTcw.at<float>(r, c) = in.pose[(size_t)(3 * r + c)];
            f.mTcw.at<float>(r, 3) = in.pose[(size_t)(9 + r)];
        }
        f.mOw = mat(in.ow.data(), 3, 1);
        f.mvScaleFactors = s.scale;
        for (float v : s.scale) { f.mvLevelSigma2.push_back(v * v); f.mvInvLevelSigma2.push_back(1.0f / (v * v)); }
        f.mnMinX = s.bounds[0]; f.mnMaxX = s.bounds[1]; f.mnMinY = s.bounds[2]; f.mnMaxY = s.bounds[3];
        f.fx = s.intr[0]; f.fy = s.intr[1]; f.cx = s.intr[2]; f.cy = s.intr[3]; f.mbf = s.intr[4];
        f.mfLogScaleFactor = s.log_scale[0];
        f.mnScaleLevels = (int)s.scale.size();
        f.mvpMapPoints.assign(n, nullptr);
        for (size_t i = 0; i < n; ++i) {
            const int32_t p = in.slot[i];
            if (p < 0) continue;
            if (p >= s.P) throw std::runtime_error("a slot names a point outside the scene");
            MapPoint &m = g.pts[(size_t)p];
            f.mvpMapPoints[i] = &m;
            if (m.mbBad || m.mObservations.count(&f)) continue;          // (a bad point keeps no observation, MapPoint.cc:201-217)
            m.mObservations[&f] = i;
            m.nObs += f.mvRight[i] >= 0 ? 2 : 1;
        }
    }
    for (int32_t k : s.targets) {
        if (k < 0 || k >= s.K) throw std::runtime_error("a target names a keyframe outside the scene");
        g.targets.push_back(&g.kfs[(size_t)k]);
        g.poses[&g.kfs[(size_t)k]] = mat(s.kf[(size_t)k].scw.data(), 4, 4);
    }
    for (int32_t i : s.list) {
        if (i >= s.P) throw std::runtime_error("the list names a point outside the scene");
        g.list.push_back(i < 0 ? nullptr : &g.pts[(size_t)i]);
    }
}

void dump(const Graph &g, const std::vector<int> &fused, BlobWriter &w) {
    std::vector<int32_t> nf(fused.begin(), fused.end());
    w.put(nf);
    const int64_t ne = (int64_t)g.log.size();
    w.put(&ne, 1);
    for (const Event &e : g.log) { const int64_t v[4] = {e.kind, e.a, e.b, e.c}; w.put(v, 4); }
    for (const KeyFrame &f : g.kfs) {
        std::vector<int32_t> slot;
        for (MapPoint *p : f.mvpMapPoints) slot.push_back(p ? (int32_t)p->mnId : -1);
        w.put(slot);
    }
    for (const MapPoint &m : g.pts) {
        const uint8_t bad = m.mbBad;
        const int32_t v[4] = {m.nObs, m.mnFound, m.mnVisible, m.mpReplaced ? (int32_t)m.mpReplaced->mnId : -1};
        w.put(&bad, 1); w.put(v, 4); w.put(m.mDescriptor.ptr(0), 32);
        const int64_t no = (int64_t)m.mObservations.size();
        w.put(&no, 1);
        for (const auto &o : m.mObservations) { const int64_t kv[2] = {(int64_t)o.first->mnId, (int64_t)o.second}; w.put(kv, 2); }
    }
}

int run(int argc, char **argv) {
    if (argc != 4) throw BlobUsage();
    const std::string mode = argv[1];
    if (mode != "fuse" && mode != "loop") throw BlobUsage();
    BlobReader r(argv[2]);
    Scene s;
    s.K = r.one<int32_t>(); s.P = r.one<int32_t>(); s.flags = r.one<int32_t>(); s.th = r.one<float>();
    if (s.K < 0 || s.P < 0) throw std::runtime_error("negative count");
    const size_t P = (size_t)s.P;
    s.intr = arr<float>(r, 5); s.bounds = arr<int32_t>(r, 4); s.scale = arr<float>(r); s.log_scale = arr<float>(r, 1);
    for (int32_t k = 0; k < s.K; ++k) {
        SceneKf f;
        f.bad = arr<uint8_t>(r, 1)[0];
        f.pose = arr<float>(r, 12); f.ow = arr<float>(r, 3); f.scw = arr<float>(r, 16);
        f.x = arr<float>(r);
        const size_t n = f.x.size();
        f.y = arr<float>(r, n); f.oct = arr<int32_t>(r, n); f.right = arr<float>(r, n); f.desc = arr<uint8_t>(r, 32 * n); f.slot = arr<int32_t>(r, n);
        s.kf.push_back(f);
    }
    s.pos = arr<float>(r, 3 * P); s.normal = arr<float>(r, 3 * P); s.mn = arr<float>(r, P); s.mx = arr<float>(r, P);
    s.desc = arr<uint8_t>(r, 32 * P); s.bad = arr<uint8_t>(r, P); s.list = arr<int32_t>(r); s.targets = arr<int32_t>(r);

    BlobWriter w;
    int32_t counts[3] = {0, 0, 0};
    {   // the adapter
        Graph g;
        build(s, g);
        log_of_current_graph() = &g.log;
        SIVO::fusion_detail::repair_switch() = !(s.flags & 1);
        const std::vector<int> fused = mode == "fuse" ? SIVO::FuseIntoKeyFrames(g.targets, g.list, s.th) : SIVO::SearchAndFuse(g.poses, g.list, &g.map, s.th);
        SIVO::fusion_detail::repair_switch() = true;
        log_of_current_graph() = nullptr;
#ifndef FUSE_BATCH_ON_LIBRARY
        counts[0] = (int32_t)fuse_batch_host::counters().batch; counts[1] = (int32_t)fuse_batch_host::counters().single;
        counts[2] = SIVO::fusion_detail::last_repairs();
#endif
        dump(g, fused, w);
        SIVO::ORBmatcher::ReleaseDeviceFrames();
    }
    {   // the loop of single-keyframe calls
        Graph g;
        build(s, g);
        log_of_current_graph() = &g.log;
        SIVO::ORBmatcher matcher(0.8f);
        std::vector<int> fused;
        if (mode == "fuse") {
            for (KeyFrame *pKFi : g.targets) fused.push_back(matcher.Fuse(pKFi, g.list, s.th));                      // LocalMapping.cc:586-594
        } else {
            for (auto mit = g.poses.begin(), mend = g.poses.end(); mit != mend; mit++) {                             // LoopClosing.cc:612-634
                KeyFrame *pKF = mit->first;
                cv::Mat cvScw = mit->second;
                std::vector<MapPoint *> vpReplacePoints(g.list.size(), static_cast<MapPoint *>(NULL));
                fused.push_back(matcher.Fuse(pKF, cvScw, g.list, s.th, vpReplacePoints));
                std::unique_lock<std::mutex> lock(g.map.mMutexMapUpdate);
                const int nLP = (int)g.list.size();
                for (int i = 0; i < nLP; i++) {
                    MapPoint *pRep = vpReplacePoints[(size_t)i];
                    if (pRep) {
                        pRep->Replace(g.list[(size_t)i]);
                    }
                }
            }
        }
        log_of_current_graph() = nullptr;
        dump(g, fused, w);
        SIVO::ORBmatcher::ReleaseDeviceFrames();
    }
    w.put(counts, 3);
    w.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "fuse_batch_adapter_prog fuse|loop IN OUT", run); }
