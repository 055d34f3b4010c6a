// ref_bawindow_driver.cpp — asks the reference's own Optimizer.cc (oracle/_ref/ref_optimizer.o, compiled untouched over the g2o stand-in of
// ref_shims_g2o) which graph Optimizer::LocalBundleAdjustment builds.  The stand-in's recording hook is handed the graph at the first
// initializeOptimization and this driver's hook leaves the function there by an exception: nothing is solved, so a scene the reference
// would not survive solving still yields its window.  Keyframes and points are the stand-ins of optimizer_standins.h; the keyframes lie
// in ONE array in ascending `addr` order, which is then the order std::map<KeyFrame *, size_t> walks them in.  Keyframe k has mnId k + 1 and
// point p mnId p (tests/localmap_restatement.py); keypoint idx of keyframe k lies at (idx, k), so an edge's measurement names its
// observation; every observation is monocular at octave 0.
//
//   ref_bawindow window IN OUT
//     in : the tables of tests/localmap_cases.tables_blob, i32 pKF, then arrays (i64 n + values): i32 cand_kf (pKF first, then its
//          ordered covisibles), i32 obs_idx (per observation, in the tables' order), i64 mnBALocalForKF and i64 mnBAFixedForKF of every
//          keyframe, i64 mnBALocalForKF of every point; then, optionally, i64 mnId of every keyframe (distinct) in place of k + 1
//     out: int64 words: n + per pose vertex in insertion order (keyframe, fixed); n + per point vertex in insertion order the point;
//          n + per edge in insertion order (position of its point vertex, position of its pose vertex, idx); then the three stamp arrays
//          as the call left them.  An edge whose second vertex is a POINT vertex (the keyframe has no pose vertex and its id is that
//          point vertex's id) carries -2 - (that point vertex's position) in place of the pose vertex
#include "include/orbslam/Optimizer.h"

#include <numeric>
#include <stdexcept>

#include "../tests/blob_io.hpp"

using namespace SIVO;

std::mutex SIVO::MapPoint::mGlobalMutex;

namespace {

template <class T> std::vector<T> arr(BlobReader &r) {
    const int64_t n = r.one<int64_t>();
    return n < 0 ? std::vector<T>() : r.many<T>((size_t)n);
}

struct Recorded {};                                                // thrown by the hook, caught below

int run(int argc, char **argv) {
    if (argc != 4 || std::string(argv[1]) != "window") throw BlobUsage();
    BlobReader r(argv[2]);
    const int32_t n_kf = r.one<int32_t>(), n_points = r.one<int32_t>();
    if (n_kf < 1 || n_points < 0) throw std::runtime_error("bad counts");
    const size_t K = (size_t)n_kf, P = (size_t)n_points;
    const std::vector<int64_t> obs_off = arr<int64_t>(r); const std::vector<int32_t> obs_kf = arr<int32_t>(r);
    const std::vector<uint8_t> point_bad = arr<uint8_t>(r), kf_bad = arr<uint8_t>(r);
    const std::vector<int64_t> slot_off = arr<int64_t>(r); const std::vector<int32_t> slot_point = arr<int32_t>(r);
    arr<int64_t>(r); arr<int32_t>(r); arr<int64_t>(r); arr<int32_t>(r); arr<int32_t>(r);      // covisibles, children, parents: cand_kf carries what is read
    const std::vector<int32_t> kf_order = arr<int32_t>(r);
    const int32_t pkf = r.one<int32_t>();
    const std::vector<int32_t> cand = arr<int32_t>(r), obs_idx = arr<int32_t>(r);
    const std::vector<int64_t> kf_local = arr<int64_t>(r), kf_fixed = arr<int64_t>(r), point_local = arr<int64_t>(r);
    std::vector<int64_t> ids = r.at != r.buf.size() ? arr<int64_t>(r) : std::vector<int64_t>();
    if (ids.empty())
        for (size_t k = 0; k < K; ++k) ids.push_back((int64_t)k + 1);
    std::map<int64_t, int64_t> kf_of_id;
    for (size_t k = 0; k < ids.size(); ++k) kf_of_id[ids[k]] = (int64_t)k;
    if (r.at != r.buf.size()) throw std::runtime_error("bytes behind the input");
    if (ids.size() != K || kf_of_id.size() != K) throw std::runtime_error("one distinct mnId per keyframe");
    if (kf_local.size() != K || kf_fixed.size() != K || point_local.size() != P || obs_idx.size() != obs_kf.size() || cand.empty() || cand[0] != pkf)
        throw std::runtime_error("inconsistent input");

    std::vector<size_t> rank(K);                                    // keyframe -> its place in the array
    if (kf_order.empty()) std::iota(rank.begin(), rank.end(), (size_t)0);
    else for (size_t i = 0; i < K; ++i) rank.at((size_t)kf_order.at(i)) = i;
    std::vector<KeyFrame> store(K);
    std::vector<MapPoint> pts(P);
    auto kf = [&](size_t k) -> KeyFrame & { return store[rank.at(k)]; };
    std::vector<size_t> keys(K);
    for (size_t k = 0; k < K; ++k) keys[k] = (size_t)(slot_off[k + 1] - slot_off[k]);
    for (size_t o = 0; o < obs_kf.size(); ++o) keys.at((size_t)obs_kf[o]) = std::max(keys[(size_t)obs_kf[o]], (size_t)obs_idx[o] + 1);
    for (size_t k = 0; k < K; ++k) {
        KeyFrame &f = kf(k);
        f.mnId = (unsigned long)ids[k]; f.mbBad = kf_bad.at(k) != 0;
        f.mnBALocalForKF = (unsigned long)kf_local[k]; f.mnBAFixedForKF = (unsigned long)kf_fixed[k];
        f.mTcw = cv::Mat::eye(4, 4, CV_32F);
        f.fx = f.fy = 500; f.cx = 320; f.cy = 240; f.mbf = 40;
        f.mvInvLevelSigma2.assign(1, 1.f);
        for (size_t s = 0; s < keys[k]; ++s) {
            cv::KeyPoint kp;
            kp.pt.x = (float)s; kp.pt.y = (float)k; kp.octave = 0;
            f.mvKeysSemantic.push_back(kp); f.mvRight.push_back(-1.f);
        }
        f.numSemanticKeys = (int)keys[k];
        for (int64_t s = slot_off[k]; s < slot_off[k + 1]; ++s) f.mvpMapPoints.push_back(slot_point[(size_t)s] < 0 ? nullptr : &pts.at((size_t)slot_point[(size_t)s]));
    }
    for (size_t i = 1; i < cand.size(); ++i) kf((size_t)pkf).mvpOrderedConnectedKeyFrames.push_back(&kf((size_t)cand[i]));
    for (size_t p = 0; p < P; ++p) {
        MapPoint &mp = pts[p];
        mp.mnId = p; mp.mbBad = point_bad.at(p) != 0; mp.mnBALocalForKF = (unsigned long)point_local[p];
        mp.mWorldPos = cv::Mat::zeros(3, 1, CV_32F);
        for (int64_t o = obs_off[p]; o < obs_off[p + 1]; ++o) mp.mObservations[&kf((size_t)obs_kf[(size_t)o])] = (size_t)obs_idx[(size_t)o];
    }

    std::vector<int64_t> w;
    bool recorded = false;
    g2o::SparseOptimizer::recordHook() = [&](const g2o::SparseOptimizer &opt) {
        std::map<const g2o::OptimizableGraph::Vertex *, int64_t> pose_at, point_at;
        std::vector<int64_t> poses, points;
        unsigned long max_id = 0;
        for (const auto *v : opt.verticesInInsertionOrder())
            if (dynamic_cast<const g2o::VertexSE3Expmap *>(v)) max_id = std::max(max_id, (unsigned long)v->id());
        for (const auto *v : opt.verticesInInsertionOrder()) {
            if (dynamic_cast<const g2o::VertexSE3Expmap *>(v)) {
                pose_at[v] = (int64_t)poses.size() / 2;
                poses.push_back(kf_of_id.at(v->id())); poses.push_back(v->fixed());
            } else {
                point_at[v] = (int64_t)points.size();
                points.push_back((int64_t)v->id() - (int64_t)max_id - 1);
            }
        }
        w.push_back((int64_t)poses.size() / 2); w.insert(w.end(), poses.begin(), poses.end());
        w.push_back((int64_t)points.size()); w.insert(w.end(), points.begin(), points.end());
        w.push_back((int64_t)opt.edges().size());
        for (const auto *e : opt.edges()) {
            const auto *pe = dynamic_cast<const g2o::ProjectionEdge *>(e);
            if (!pe || !point_at.count(e->vertex(0))) throw std::runtime_error("an edge that is none of the window's");
            const int64_t idx = (int64_t)pe->measurement()[0], k = (int64_t)pe->measurement()[1];
            // optimizer.vertex(pKFi->mnId) looks the keyframe's id up among ALL vertices (Optimizer.cc:687, :726): a keyframe without a
            // pose vertex whose id is a point vertex's gets that one.  Written as -2 - (position of the point vertex).
            int64_t second;
            if (pose_at.count(e->vertex(1))) {
                if (k != kf_of_id.at(e->vertex(1)->id())) throw std::runtime_error("an edge's measurement is not its keyframe's");
                second = pose_at[e->vertex(1)];
            } else {
                if (!point_at.count(e->vertex(1)) || ids.at((size_t)k) != e->vertex(1)->id()) throw std::runtime_error("an edge that is none of the window's");
                second = -2 - point_at[e->vertex(1)];
            }
            w.push_back(point_at[e->vertex(0)]); w.push_back(second); w.push_back(idx);
        }
        recorded = true;
        throw Recorded{};
    };
    try {
        RefOptimizer::LocalBundleAdjustment(&kf((size_t)pkf), nullptr, nullptr);
    } catch (const Recorded &) {
    }
    g2o::SparseOptimizer::recordHook() = nullptr;
    if (!recorded) throw std::runtime_error("LocalBundleAdjustment returned without initializeOptimization");
    for (size_t k = 0; k < K; ++k) w.push_back((int64_t)kf(k).mnBALocalForKF);
    for (size_t k = 0; k < K; ++k) w.push_back((int64_t)kf(k).mnBAFixedForKF);
    for (size_t p = 0; p < P; ++p) w.push_back((int64_t)pts[p].mnBALocalForKF);
    BlobWriter o;
    o.put(w);
    o.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "ref_bawindow window IN OUT", run); }
