// ref_loopclosing_driver.cpp — feeds the reference's own LoopClosing.cc, KeyFrame.cc, MapPoint.cc, Map.cc and Converter.cc (compiled
// untouched with their own headers, see the Makefile) the scenes of tests/loop_closing_pin_cases.py and writes what they leave.  The objects
// are REAL KeyFrame / MapPoint / Map / LoopClosing objects; protected state is reached through the derived classes below, nothing is #defined
// over the sources.  Keyframes are allocated from the arena of ref_arena.inc in ascending `addr` order, so the order in which
// std::map<KeyFrame *, g2o::Sim3> and std::set<KeyFrame *> walk them is the scene's `addr` order; one more keyframe, the ANCHOR, is allocated
// behind them (index n_kf in every output) and is only the reference keyframe a MapPoint's constructor asks for.  Keypoint `idx` of keyframe
// k lies at (idx, k).  One routine per invocation:
//
//   ref_loopclosing loop IN OUT : the graph blob of tests/covis_adapter_cases.graph_blob (every keyframe, the ones outside the corrected set
//       included), then addr i64[K], scale factors f32[8], Tcw f32[K][16], descriptors u8[slots][32], position f32[P][3], reference
//       keyframe i32[P], corrected-by-this-loop u8[P], i32 current, i32 matched, mg2oScw f64[8] (qx qy qz qw tx ty tz s), i32 n +
//       mvpCurrentMatchedPoints i32[n] (-1: none), i32 n + mvpLoopMapPoints i32[n], i32 n + the matcher's script i32[n][3] (keyframe, index
//       into mvpLoopMapPoints, slot).  LoopClosing::CorrectLoop() whole.  Optimizer::OptimizeEssentialGraph (a stand-in) is the snapshot
//       point: every pose, centre, position, normal, distance, slot, observation, descriptor and flag as correction, loop fusion and
//       SearchAndFuse left them, with the two Sim3 maps in map order and LoopConnections.  Optimizer::GlobalBundleAdjustment sets the stop
//       flag, so the thread of :600 skips the map update; it is joined before anything else is read.
//   ref_loopclosing fuse IN OUT : i32 K, i32 P, slot offsets i64[K + 1], the point per slot i32[slots], mvRight f32[slots], descriptors
//       u8[slots][32], per point bad u8[P] and descriptor u8[P][32], i32 n + mvpLoopMapPoints i32[n], i32 n + the keyframes of
//       CorrectedPosesMap i32[n], i32 n + the matcher's script i32[n][3].  The keyframes lie in index order; a point that is not bad is
//       observed by every keyframe that holds it, at its first slot there.  LoopClosing::SearchAndFuse(CorrectedPosesMap) alone, every
//       pose the identity (the scripted matcher reads none) -> the graph it leaves, as `loop` writes it.
//   ref_loopclosing gba IN OUT  : i32 K, i32 P, i32 n_origins, i64 nLoopKF, addr i64[K], id i64[K], Tcw / mTcwGBA / mTcwBefGBA f32[K][16] each,
//       mnBAGlobalForKF i64[K], parent i32[K] (-1: none), origins i32[n_origins], position / mPosGBA f32[P][3] each, mnBAGlobalForKF
//       i64[P], bad u8[P], reference keyframe i32[P].  LoopClosing::RunGlobalBundleAdjustment(nLoopKF), called directly.
//   output: records of (name length i32, name, element size i32, count i64, bytes), which tests/loop_closing_pin_cases.py reads by name.
#include <unistd.h>
#include <cstdlib>
#include <cstdio>

#include "include/orbslam/LoopClosing.h"
#include "include/orbslam/Converter.h"

#include <cstring>
#include <numeric>
#include <stdexcept>

#include "../tests/blob_io.hpp"
#include "ref_arena.inc"

using namespace SIVO;

long unsigned int Frame::nNextId = 0;
bool Frame::mbInitialComputations = true;

namespace {

struct KF : KeyFrame {
    KF(Frame &F, Map *pMap, KeyFrameDatabase *pKFDB) : KeyFrame(F, pMap, pKFDB) {}
    using KeyFrame::mbBad;
    using KeyFrame::mbFirstConnection;
    using KeyFrame::mbToBeErased;
    using KeyFrame::mConnectedKeyFrameWeights;
    using KeyFrame::mpParent;
    using KeyFrame::mspChildren;
    using KeyFrame::mspLoopEdges;
    using KeyFrame::mvOrderedWeights;
    using KeyFrame::mvpMapPoints;
    using KeyFrame::mvpOrderedConnectedKeyFrames;
};
struct MP : MapPoint {
    MP(const cv::Mat &Pos, KeyFrame *pRefKF, Map *pMap) : MapPoint(Pos, pRefKF, pMap) {}
    using MapPoint::mbBad;
    using MapPoint::mDescriptor;
    using MapPoint::mfMaxDistance;
    using MapPoint::mfMinDistance;
    using MapPoint::mnFound;
    using MapPoint::mNormalVector;
    using MapPoint::mnVisible;
    using MapPoint::mObservations;
    using MapPoint::mpRefKF;
    using MapPoint::mpReplaced;
    using MapPoint::mWorldPos;
};
struct LC : LoopClosing {
    LC(Map *pMap, KeyFrameDatabase *pDB, ORBVocabulary *pVoc) : LoopClosing(pMap, pDB, pVoc, true) {}
    using LoopClosing::CorrectLoop;
    using LoopClosing::mg2oScw;
    using LoopClosing::mLastLoopKFid;
    using LoopClosing::mpCurrentKF;
    using LoopClosing::mpMatchedKF;
    using LoopClosing::mpThreadGBA;
    using LoopClosing::mvpCurrentConnectedKFs;
    using LoopClosing::mvpCurrentMatchedPoints;
    using LoopClosing::mvpLoopMapPoints;
    using LoopClosing::SearchAndFuse;
    void join() {
        if (mpThreadGBA) { mpThreadGBA->join(); delete mpThreadGBA; mpThreadGBA = nullptr; }
    }
};

cv::Mat pose_of(const float *t) {
    cv::Mat T(4, 4, CV_32F);
    for (int i = 0; i < 16; ++i) T.at<float>(i / 4, i % 4) = t[i];
    return T;
}
cv::Mat vec3_of(const float *p) {
    cv::Mat v(3, 1, CV_32F);
    for (int i = 0; i < 3; ++i) v.at<float>(i) = p[i];
    return v;
}

struct Out : BlobWriter {
    template <class T> void rec(const char *name, const std::vector<T> &v) {
        const int32_t n = (int32_t)std::strlen(name), size = (int32_t)sizeof(T);
        const int64_t count = (int64_t)v.size();
        put(&n, 1); put(name, (size_t)n); put(&size, 1); put(&count, 1); put(v);
    }
};

// the world of one run: keyframes in arena order of their addr, the anchor behind them, points in index order
struct World {
    Map map;
    KeyFrameDatabase db;
    ORBVocabulary voc;
    std::vector<KF *> kfs;
    std::vector<MP *> pts;
    KF *anchor = nullptr;
    std::map<const KeyFrame *, int32_t> kf_index;
    std::map<const MapPoint *, int32_t> pt_index;

    // fill(k, F): what the Frame the keyframe is made from carries beside its id
    template <class Fill> void make_keyframes(const std::vector<int64_t> &ids, const std::vector<int64_t> &addr, Fill fill) {
        const size_t K = ids.size();
        std::vector<size_t> order(K);
        std::iota(order.begin(), order.end(), (size_t)0);
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return addr[a] < addr[b]; });
        for (size_t i = 1; i < K; ++i)
            if (addr[order[i]] == addr[order[i - 1]]) throw std::runtime_error("two keyframes at one addr");
        kfs.assign(K, nullptr);
        arena_begin(true);
        for (size_t i = 0; i <= K; ++i) {
            const bool is_anchor = i == K;
            const size_t k = is_anchor ? K : order[i];
            Frame F;
            F.mnId = 1000 + k;
            if (!is_anchor) fill(k, F);
            F.numSemanticKeys = (int)F.mvKeysSemantic.size();
            F.mvpMapPoints.assign(F.mvKeysSemantic.size(), nullptr);
            KeyFrame::nNextId = is_anchor ? (1ul << 20) : (unsigned long)ids[k];
            KF *kf = new KF(F, &map, &db);
            if (is_anchor) anchor = kf; else kfs[k] = kf;
        }
        for (size_t i = 1; i < K; ++i)
            if (!(kfs[order[i - 1]] < kfs[order[i]])) throw std::runtime_error("the arena did not keep the addr order");
        if (K && !(kfs[order[K - 1]] < anchor)) throw std::runtime_error("the anchor is not behind the keyframes");
        for (size_t k = 0; k < K; ++k) {
            if (kfs[k]->mnId != (unsigned long)ids[k]) throw std::runtime_error("mnId was not taken from nNextId");
            kf_index[kfs[k]] = (int32_t)k;
        }
        kf_index[anchor] = (int32_t)K;
    }
    void make_points(const std::vector<float> &pos) {
        MapPoint::nNextId = 0;
        for (size_t p = 0; p < pos.size() / 3; ++p) {
            pts.push_back(new MP(vec3_of(&pos[3 * p]), anchor, &map));
            pt_index[pts.back()] = (int32_t)p;
        }
        arena_on = false;                                      // from here on the heap: what the routines allocate is the sanitizers' to watch
    }
    int32_t ik(const KeyFrame *kf) const {
        if (!kf) return -1;
        auto it = kf_index.find(kf);
        if (it == kf_index.end()) throw std::runtime_error("a keyframe that is not the scene's");
        return it->second;
    }
    int32_t ip(const MapPoint *p) const {
        if (!p) return -1;
        auto it = pt_index.find(p);
        if (it == pt_index.end()) throw std::runtime_error("a point that is not the scene's");
        return it->second;
    }
    // the int32 stream of tests/covis_adapter_prog.cpp's Graph::dump
    void dump(std::vector<int32_t> &w) const {
        for (const KF *kf : kfs) {
            w.push_back(kf->mbBad); w.push_back(kf->mbToBeErased); w.push_back(kf->mbFirstConnection); w.push_back(ik(kf->mpParent));
            w.push_back((int32_t)kf->mvpOrderedConnectedKeyFrames.size());
            for (const KeyFrame *o : kf->mvpOrderedConnectedKeyFrames) w.push_back(ik(o));
            w.push_back((int32_t)kf->mvOrderedWeights.size());
            for (int x : kf->mvOrderedWeights) w.push_back(x);
            w.push_back((int32_t)kf->mConnectedKeyFrameWeights.size());
            for (const auto &kw : kf->mConnectedKeyFrameWeights) { w.push_back(ik(kw.first)); w.push_back(kw.second); }
            w.push_back((int32_t)kf->mspChildren.size());
            for (const KeyFrame *c : kf->mspChildren) w.push_back(ik(c));
            w.push_back((int32_t)kf->mvpMapPoints.size());
            for (const MapPoint *p : kf->mvpMapPoints) w.push_back(ip(p));
        }
        for (MP *mp : pts) {
            w.push_back(mp->mbBad); w.push_back(mp->Observations()); w.push_back((int32_t)mp->mObservations.size());
            for (const auto &ob : mp->mObservations) { w.push_back(ik(ob.first)); w.push_back((int32_t)ob.second); }
        }
    }
    void poses(Out &o, const char *tcw, const char *ow) const {
        std::vector<float> t, c;
        for (KF *kf : kfs) {
            const cv::Mat T = kf->GetPose(), O = kf->GetCameraCenter();
            for (int i = 0; i < 16; ++i) t.push_back(T.at<float>(i / 4, i % 4));
            for (int i = 0; i < 3; ++i) c.push_back(O.at<float>(i));
        }
        o.rec(tcw, t); o.rec(ow, c);
    }
    // every point and the graph as they stand: position, normal, distances, flags, marks, descriptor; slots and observations (`dump`)
    void graph(Out &o) const {
        std::vector<float> xyz, normal, dmin, dmax;
        std::vector<uint8_t> flag, has_desc, d;
        std::vector<int64_t> by, reference;
        std::vector<int32_t> replaced, fv;
        for (MP *mp : pts) {
            for (int i = 0; i < 3; ++i) { xyz.push_back(mp->mWorldPos.at<float>(i)); normal.push_back(mp->mNormalVector.at<float>(i)); }
            dmin.push_back(mp->mfMinDistance); dmax.push_back(mp->mfMaxDistance);
            flag.push_back(mp->mbBad);
            by.push_back((int64_t)mp->mnCorrectedByKF); reference.push_back((int64_t)mp->mnCorrectedReference);
            replaced.push_back(ip(mp->mpReplaced));
            fv.push_back(mp->mnFound); fv.push_back(mp->mnVisible);
            has_desc.push_back(!mp->mDescriptor.empty());
            for (int i = 0; i < 32; ++i) d.push_back(mp->mDescriptor.empty() ? 0 : mp->mDescriptor.ptr<unsigned char>()[i]);
        }
        o.rec("pos", xyz); o.rec("normal", normal); o.rec("min_dist", dmin); o.rec("max_dist", dmax); o.rec("bad", flag);
        o.rec("corrected_by_id", by); o.rec("corrected_reference_id", reference); o.rec("replaced", replaced); o.rec("found_visible", fv);
        o.rec("has_descriptor", has_desc); o.rec("descriptor", d);
        std::vector<int32_t> w;
        dump(w);
        o.rec("dump", w);
    }
    // the calls the scripted matcher met, in order
    void fuse_calls(Out &o) const {
        std::vector<int32_t> kf, action;
        std::vector<float> scw;
        std::vector<uint8_t> desc;
        for (const FuseScript::Call &c : FuseScript::get().calls) {
            kf.push_back(ik(c.kf));
            scw.insert(scw.end(), c.scw, c.scw + 16);
            action.insert(action.end(), c.action.begin(), c.action.end());
            desc.insert(desc.end(), c.descriptor.begin(), c.descriptor.end());
        }
        o.rec("fuse_kf", kf); o.rec("fuse_scw", scw); o.rec("fuse_action", action); o.rec("fuse_descriptor", desc);
    }
    ~World() {                                                  // the objects lie in the arena; what they hold on the heap goes back
        for (MP *p : pts) p->~MP();
        for (KF *k : kfs) k->~KF();
        if (anchor) anchor->~KF();
        arena_end();
    }
};

void put_sim3(std::vector<double> &v, const g2o::Sim3 &S) {
    v.push_back(S.rotation().x()); v.push_back(S.rotation().y()); v.push_back(S.rotation().z()); v.push_back(S.rotation().w());
    for (int i = 0; i < 3; ++i) v.push_back(S.translation()(i));
    v.push_back(S.scale());
}

int run_loop(const char *in, const char *out) {
    BlobReader r(in);
    const int32_t n_kf = r.one<int32_t>(), n_points = r.one<int32_t>();
    if (n_kf < 1 || n_points < 0) throw std::runtime_error("bad count");
    const size_t K = (size_t)n_kf, P = (size_t)n_points;
    const std::vector<int64_t> ids = r.many<int64_t>(K);
    r.many<uint8_t>(K);                                        // (mbNotErase: CorrectLoop does not read it)
    r.many<float>(K);                                          // (mThDepth: likewise)
    const std::vector<int64_t> slot_off = r.many<int64_t>(K + 1);
    const size_t ns = (size_t)slot_off[K];
    const std::vector<int32_t> slot_point = r.many<int32_t>(ns);
    const std::vector<uint8_t> slot_level = r.many<uint8_t>(ns);
    const std::vector<float> slot_right = r.many<float>(ns), slot_depth = r.many<float>(ns);
    const std::vector<uint8_t> bad = r.many<uint8_t>(P);
    const std::vector<int32_t> found = r.many<int32_t>(P), visible = r.many<int32_t>(P);
    r.many<int64_t>(P);                                        // (mnFirstKFid)
    r.many<int32_t>(P);                                        // (nObs: AddObservation counts it)
    const std::vector<int64_t> obs_off = r.many<int64_t>(P + 1);
    const std::vector<int32_t> obs_kf = r.many<int32_t>((size_t)obs_off[P]), obs_idx = r.many<int32_t>((size_t)obs_off[P]);
    const std::vector<int64_t> addr = r.many<int64_t>(K);
    const std::vector<float> sf = r.many<float>(8), tcw = r.many<float>(16 * K);
    const std::vector<uint8_t> desc = r.many<uint8_t>(32 * ns);
    const std::vector<float> pos = r.many<float>(3 * P);
    const std::vector<int32_t> ref = r.many<int32_t>(P);
    const std::vector<uint8_t> corrected = r.many<uint8_t>(P);
    const int32_t cur = r.one<int32_t>(), matched = r.one<int32_t>();
    const std::vector<double> scw = r.many<double>(8);
    const std::vector<int32_t> cur_matched = r.many<int32_t>((size_t)r.one<int32_t>());
    const std::vector<int32_t> loop_points = r.many<int32_t>((size_t)r.one<int32_t>());
    const std::vector<int32_t> script = r.many<int32_t>(3 * (size_t)r.one<int32_t>());
    if (r.at != r.buf.size()) throw std::runtime_error("bytes behind the scene");

    World W;
    W.make_keyframes(ids, addr, [&](size_t k, Frame &F) {
        const size_t n = (size_t)(slot_off[k + 1] - slot_off[k]);
        F.mDescriptorsSemantic = cv::Mat(cv::Mat::zeros((int)n, 32, CV_8U));
        for (size_t s = 0; s < n; ++s) {
            const size_t at = (size_t)slot_off[k] + s;
            cv::KeyPoint kp;
            kp.pt.x = (float)s; kp.pt.y = (float)k; kp.octave = slot_level[at];
            F.mvKeysSemantic.push_back(kp);
            F.mvRight.push_back(slot_right[at]);
            F.mvDepth.push_back(slot_depth[at]);
            std::memcpy(F.mDescriptorsSemantic.ptr<unsigned char>((int)s), &desc[32 * at], 32);
        }
        F.mnScaleLevels = (int)sf.size();
        F.mvScaleFactors = sf;
        F.mTcw = pose_of(&tcw[16 * k]);
    });
    W.make_points(pos);
    for (size_t k = 0; k < K; ++k)
        for (int64_t s = slot_off[k]; s < slot_off[k + 1]; ++s)
            if (slot_point[(size_t)s] >= 0) W.kfs[k]->AddMapPoint(W.pts.at((size_t)slot_point[(size_t)s]), (size_t)(s - slot_off[k]));
    KF *current = W.kfs.at((size_t)cur);
    for (size_t p = 0; p < P; ++p) {
        MP *mp = W.pts[p];
        mp->mnFound = found[p]; mp->mnVisible = visible[p];
        for (int64_t o = obs_off[p]; o < obs_off[p + 1]; ++o) {
            KF *kf = W.kfs.at((size_t)obs_kf[(size_t)o]);
            if ((size_t)obs_idx[(size_t)o] >= kf->mvRight.size()) throw std::runtime_error("an observation's idx is no slot of its keyframe");
            mp->AddObservation(kf, (size_t)obs_idx[(size_t)o]);
        }
        mp->mpRefKF = W.kfs.at((size_t)ref[p]);
        mp->ComputeDistinctiveDescriptors();                   // the descriptor the point came with: the reference's choice among its observations
        mp->mbBad = bad[p] != 0;
        if (corrected[p]) mp->mnCorrectedByKF = current->mnId;
        W.map.AddMapPoint(mp);
    }
    for (KF *kf : W.kfs) W.map.AddKeyFrame(kf);

    LocalMapping mapper;
    LC lc(&W.map, &W.db, &W.voc);
    lc.SetLocalMapper(&mapper);
    lc.mpCurrentKF = current;
    lc.mpMatchedKF = W.kfs.at((size_t)matched);
    lc.mg2oScw = g2o::Sim3(Eigen::Quaterniond(scw[3], scw[0], scw[1], scw[2]), Eigen::Vector3d(scw[4], scw[5], scw[6]), scw[7]);
    for (int32_t p : cur_matched) lc.mvpCurrentMatchedPoints.push_back(p < 0 ? nullptr : W.pts.at((size_t)p));
    for (int32_t p : loop_points) lc.mvpLoopMapPoints.push_back(W.pts.at((size_t)p));
    for (size_t i = 0; i < script.size(); i += 3)
        FuseScript::get().landings[W.kfs.at((size_t)script[i])].push_back(FuseScript::Landing{script[i + 1], script[i + 2]});

    Out o;
    int snapshots = 0;
    Optimizer::stop_global_ba() = true;
    Optimizer::on_essential_graph() = [&](const LoopClosing::KeyFrameAndPose &non, const LoopClosing::KeyFrameAndPose &cor,
                                          const std::map<KeyFrame *, std::set<KeyFrame *> > &conn) {
        ++snapshots;
        std::vector<int32_t> kf;
        std::vector<double> s;
        for (const auto &e : cor) { kf.push_back(W.ik(e.first)); put_sim3(s, e.second); }
        o.rec("corrected_kf", kf); o.rec("corrected_sim3", s);
        kf.clear(); s.clear();
        for (const auto &e : non) { kf.push_back(W.ik(e.first)); put_sim3(s, e.second); }
        o.rec("noncorrected_kf", kf); o.rec("noncorrected_sim3", s);
        std::vector<int32_t> c;
        for (const auto &e : conn) {
            c.push_back(W.ik(e.first)); c.push_back((int32_t)e.second.size());
            for (const KeyFrame *k2 : e.second) c.push_back(W.ik(k2));
        }
        o.rec("loop_connections", c);
        W.poses(o, "tcw", "ow");
        W.graph(o);
    };
    lc.CorrectLoop();
    lc.join();
    if (snapshots != 1) throw std::runtime_error("OptimizeEssentialGraph was not called once");

    std::vector<int32_t> v;
    for (const KeyFrame *kf : lc.mvpCurrentConnectedKFs) v.push_back(W.ik(kf));
    o.rec("connected", v);
    W.fuse_calls(o);
    v.clear();
    for (const KF *kf : W.kfs) {
        v.push_back((int32_t)kf->mspLoopEdges.size());
        for (const KeyFrame *e : kf->mspLoopEdges) v.push_back(W.ik(e));
    }
    o.rec("loop_edges", v);
    v = {mapper.n_request_stop, mapper.n_release, Optimizer::global_ba_calls(), (int32_t)lc.mLastLoopKFid, (int32_t)lc.isRunningGBA(),
         W.map.GetLastBigChangeIdx()};
    o.rec("after", v);
    o.save(out);
    return 0;
}

int run_fuse(const char *in, const char *out) {
    BlobReader r(in);
    const int32_t n_kf = r.one<int32_t>(), n_points = r.one<int32_t>();
    if (n_kf < 0 || n_points < 0) throw std::runtime_error("negative count");
    const size_t K = (size_t)n_kf, P = (size_t)n_points;
    const std::vector<int64_t> slot_off = r.many<int64_t>(K + 1);
    const size_t ns = (size_t)slot_off[K];
    const std::vector<int32_t> slot_point = r.many<int32_t>(ns);
    const std::vector<float> slot_right = r.many<float>(ns);
    const std::vector<uint8_t> desc = r.many<uint8_t>(32 * ns), bad = r.many<uint8_t>(P), point_desc = r.many<uint8_t>(32 * P);
    const std::vector<int32_t> loop_points = r.many<int32_t>((size_t)r.one<int32_t>());
    const std::vector<int32_t> targets = r.many<int32_t>((size_t)r.one<int32_t>());
    const std::vector<int32_t> script = r.many<int32_t>(3 * (size_t)r.one<int32_t>());
    if (r.at != r.buf.size()) throw std::runtime_error("bytes behind the scene");

    std::vector<int64_t> ids(K), addr(K);
    for (size_t k = 0; k < K; ++k) { ids[k] = 100 + (int64_t)k; addr[k] = (int64_t)k; }
    World W;
    W.make_keyframes(ids, addr, [&](size_t k, Frame &F) {
        const size_t n = (size_t)(slot_off[k + 1] - slot_off[k]);
        F.mDescriptorsSemantic = cv::Mat(cv::Mat::zeros((int)n, 32, CV_8U));
        for (size_t s = 0; s < n; ++s) {
            const size_t at = (size_t)slot_off[k] + s;
            cv::KeyPoint kp;
            kp.pt.x = (float)s; kp.pt.y = (float)k; kp.octave = 0;
            F.mvKeysSemantic.push_back(kp);
            F.mvRight.push_back(slot_right[at]);
            F.mvDepth.push_back(1.f);
            std::memcpy(F.mDescriptorsSemantic.ptr<unsigned char>((int)s), &desc[32 * at], 32);
        }
    });
    W.make_points(std::vector<float>(3 * P, 0.f));
    for (size_t p = 0; p < P; ++p) {
        W.pts[p]->mDescriptor = cv::Mat(cv::Mat::zeros(1, 32, CV_8U));
        std::memcpy(W.pts[p]->mDescriptor.ptr<unsigned char>(0), &point_desc[32 * p], 32);
        W.map.AddMapPoint(W.pts[p]);
    }
    for (size_t k = 0; k < K; ++k)
        for (int64_t s = slot_off[k]; s < slot_off[k + 1]; ++s) {
            const int32_t p = slot_point[(size_t)s];
            if (p < 0) continue;
            W.kfs[k]->AddMapPoint(W.pts.at((size_t)p), (size_t)(s - slot_off[k]));
            if (!bad[(size_t)p]) W.pts[(size_t)p]->AddObservation(W.kfs[k], (size_t)(s - slot_off[k]));      // (the first slot: :151 passes a second one over)
        }
    for (size_t p = 0; p < P; ++p) W.pts[p]->mbBad = bad[p] != 0;

    LocalMapping mapper;
    LC lc(&W.map, &W.db, &W.voc);
    lc.SetLocalMapper(&mapper);
    for (int32_t p : loop_points) lc.mvpLoopMapPoints.push_back(W.pts.at((size_t)p));
    LoopClosing::KeyFrameAndPose poses;
    for (int32_t k : targets) poses[W.kfs.at((size_t)k)] = g2o::Sim3();
    for (size_t i = 0; i < script.size(); i += 3)
        FuseScript::get().landings[W.kfs.at((size_t)script[i])].push_back(FuseScript::Landing{script[i + 1], script[i + 2]});
    lc.SearchAndFuse(poses);

    Out o;
    W.graph(o);
    W.fuse_calls(o);
    o.save(out);
    return 0;
}

int run_gba(const char *in, const char *out) {
    BlobReader r(in);
    const int32_t n_kf = r.one<int32_t>(), n_points = r.one<int32_t>(), n_origins = r.one<int32_t>();
    const int64_t loop_kf = r.one<int64_t>();
    if (n_kf < 0 || n_points < 0 || n_origins < 0) throw std::runtime_error("negative count");
    const size_t K = (size_t)n_kf, P = (size_t)n_points;
    const std::vector<int64_t> addr = r.many<int64_t>(K), ids = r.many<int64_t>(K);
    const std::vector<float> tcw = r.many<float>(16 * K), gba = r.many<float>(16 * K), bef = r.many<float>(16 * K);
    const std::vector<int64_t> kf_ba = r.many<int64_t>(K);
    const std::vector<int32_t> parent = r.many<int32_t>(K), origins = r.many<int32_t>((size_t)n_origins);
    const std::vector<float> pos = r.many<float>(3 * P), pos_gba = r.many<float>(3 * P);
    const std::vector<int64_t> pt_ba = r.many<int64_t>(P);
    const std::vector<uint8_t> bad = r.many<uint8_t>(P);
    const std::vector<int32_t> ref = r.many<int32_t>(P);
    if (r.at != r.buf.size()) throw std::runtime_error("bytes behind the scene");

    World W;
    W.make_keyframes(ids, addr, [&](size_t k, Frame &F) { F.mTcw = pose_of(&tcw[16 * k]); });
    W.make_points(pos);
    for (size_t k = 0; k < K; ++k) {
        KF *kf = W.kfs[k];
        kf->mTcwGBA = pose_of(&gba[16 * k]);
        kf->mTcwBefGBA = pose_of(&bef[16 * k]);
        kf->mnBAGlobalForKF = (unsigned long)kf_ba[k];
        if (parent[k] >= 0) kf->ChangeParent(W.kfs.at((size_t)parent[k]));
        W.map.AddKeyFrame(kf);
    }
    for (int32_t k : origins) W.map.mvpKeyFrameOrigins.push_back(W.kfs.at((size_t)k));
    for (size_t p = 0; p < P; ++p) {
        MP *mp = W.pts[p];
        mp->mPosGBA = vec3_of(&pos_gba[3 * p]);
        mp->mnBAGlobalForKF = (unsigned long)pt_ba[p];
        mp->mpRefKF = W.kfs.at((size_t)ref[p]);
        mp->mbBad = bad[p] != 0;
        W.map.AddMapPoint(mp);
    }
    LocalMapping mapper;
    LC lc(&W.map, &W.db, &W.voc);
    lc.SetLocalMapper(&mapper);
    Optimizer::stop_global_ba() = false;
    lc.RunGlobalBundleAdjustment((unsigned long)loop_kf);

    Out o;
    W.poses(o, "tcw", "ow");
    std::vector<float> g, b, xyz;
    std::vector<int64_t> ba;
    for (KF *kf : W.kfs) {
        for (int i = 0; i < 16; ++i) { g.push_back(kf->mTcwGBA.at<float>(i / 4, i % 4)); b.push_back(kf->mTcwBefGBA.at<float>(i / 4, i % 4)); }
        ba.push_back((int64_t)kf->mnBAGlobalForKF);
    }
    for (MP *mp : W.pts)
        for (int i = 0; i < 3; ++i) xyz.push_back(mp->mWorldPos.at<float>(i));
    o.rec("tcw_gba", g); o.rec("tcw_bef", b); o.rec("kf_ba", ba); o.rec("pos", xyz);
    std::vector<int32_t> v = {mapper.n_request_stop, mapper.n_release, Optimizer::global_ba_calls(), (int32_t)lc.isFinishedGBA(),
                              W.map.GetLastBigChangeIdx()};
    o.rec("after", v);
    o.save(out);
    return 0;
}

int run(int argc, char **argv) {
    if (argc != 4) throw BlobUsage();
    const std::string mode = argv[1];
    if (mode == "loop") return run_loop(argv[2], argv[3]);
    if (mode == "gba") return run_gba(argv[2], argv[3]);
    if (mode == "fuse") return run_fuse(argv[2], argv[3]);
    throw BlobUsage();
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "ref_loopclosing loop|gba|fuse IN OUT", run); }
