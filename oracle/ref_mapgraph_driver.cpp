// ref_mapgraph_driver.cpp — feeds the reference's own KeyFrame.cc, MapPoint.cc, Map.cc, LocalMapping.cc and Tracking.cc (compiled untouched
// with their own headers, see the Makefile) the scenes of tests/map_graph_pin_cases.py and writes what they leave.  The objects are REAL
// KeyFrame / MapPoint / Map / LocalMapping / Tracking objects; protected state is reached through the derived classes below, nothing is
// #defined over the sources.  Keyframes are allocated from the arena of ref_arena.inc in ascending `addr` order, so the order in which
// std::map<KeyFrame *, ...> and std::set<KeyFrame *> walk them is the scene's `addr` order; one more keyframe, the ANCHOR, is allocated
// behind them (index n_kf in every output): it is the reference keyframe of every point (so MapPoint.cc:177-178 never picks another), the
// current keyframe of the two culling calls, and the parent of a keyframe the scene gives none where SetBadFlag needs one
// (KeyFrame.cc:505, :530, :561 dereference it).  Keypoint `idx` of keyframe k lies at (idx, k): distinct coordinates.
//
//   graph   : the blob of tests/covis_adapter_cases.graph_blob (tests/covis_adapter_prog.cpp states it)
//   trailer : addr i64[n_kf], kf_bad u8[n_kf], i32 links; with links: parent i32[n_kf] (-1: none), first_connection u8[n_kf],
//             w_off i64[n_kf + 1], w_kf i32[..], w_val i32[..] (mConnectedKeyFrameWeights per keyframe; the ordered vectors follow from
//             KeyFrame::UpdateBestCovisibles, the children from the parents)
//   dump    : the int32 stream of covis_adapter_prog.cpp's Graph::dump, the anchor written as n_kf
//
//   ref_mapgraph connections IN OUT : graph, i32 n, order i32[n], trailer.  KeyFrame::UpdateConnections per entry of `order` -> dump
//   ref_mapgraph kfcull IN OUT      : graph, i32 mono, i32 n, local i32[n], trailer.  Without links every keyframe's parent is the anchor.
//                                     LocalMapping::KeyFrameCulling -> dump, i32 n + the KeyFrameDatabase::erase calls in order
//   ref_mapgraph mpcull IN OUT      : graph, i32 mono, i64 current id, i32 n, list i32[n], trailer.  LocalMapping::MapPointCulling -> dump,
//                                     i32 n + mlpRecentAddedMapPoints afterwards
//   ref_mapgraph chain IN OUT       : graph, i32 mono, i32 frame id, i32 n, frame slots i32[n], trailer.  Nothing is connected by hand:
//                                     UpdateConnections of every keyframe in mnId order -> i32 n + dump; KeyFrameCulling from the keyframe
//                                     of the largest mnId (its own ordered covisibles are the list) -> i32 n + dump, i32 n + the erase
//                                     calls; UpdateLocalMap for the frame, with no list and no reference keyframe held -> i32 n + local
//                                     keyframes, i32 n + local points, pReferenceKF, F.mpReferenceKF, the frame's slots, then
//                                     mnTrackReferenceForFrame of every keyframe and point (i32)
//   ref_mapgraph localmap IN OUT    : the blob of tests/localmap_cases.adapter_blob (tests/localmap_adapter_prog.cpp states it; unknown_slot,
//                                     bad_kfs and bad_points must be empty).  Tracking::UpdateLocalMap -> what localmap_adapter_prog writes
#include <unistd.h>
#include <cstdlib>
#include <cstdio>

#include "include/orbslam/Tracking.h"

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
    using KeyFrame::mbNotErase;
    using KeyFrame::mbToBeErased;
    using KeyFrame::mConnectedKeyFrameWeights;
    using KeyFrame::mpParent;
    using KeyFrame::mspChildren;
    using KeyFrame::mvOrderedWeights;
    using KeyFrame::mvpMapPoints;
    using KeyFrame::mvpOrderedConnectedKeyFrames;
};
struct MP : MapPoint {
    MP(const cv::Mat &Pos, KeyFrame *pRefKF, Map *pMap) : MapPoint(Pos, pRefKF, pMap) {}
    using MapPoint::mbBad;
    using MapPoint::mnFound;
    using MapPoint::mnVisible;
    using MapPoint::mObservations;
};
struct LM : LocalMapping {
    LM(Map *pMap, bool mono) : LocalMapping(pMap, mono) {}
    using LocalMapping::KeyFrameCulling;
    using LocalMapping::MapPointCulling;
    using LocalMapping::mlpRecentAddedMapPoints;
    using LocalMapping::mpCurrentKeyFrame;
};
struct TR : Tracking {
    TR(Map *pMap, KeyFrameDatabase *pKFDB) : Tracking(nullptr, nullptr, nullptr, nullptr, pMap, pKFDB, nullptr, "settings", System::STEREO) {}
    using Tracking::mpReferenceKF;
    using Tracking::mvpLocalKeyFrames;
    using Tracking::mvpLocalMapPoints;
    using Tracking::UpdateLocalMap;
    ~TR() { delete mpORBextractorLeft; delete mpORBextractorRight; }       // (the constructor's two, which the class never frees)
};

// the world of one run: keyframes in arena order of their addr, the anchor behind them, points in index order
struct World {
    Map map;
    KeyFrameDatabase db;
    std::vector<KF *> kfs;
    std::vector<MP *> pts;
    KF *anchor = nullptr;

    // per keyframe: id, addr, and per slot octave / right / depth
    void make_keyframes(const std::vector<int64_t> &ids, const std::vector<int64_t> &addr, const std::vector<int64_t> &slot_off,
                        const uint8_t *level, const float *right, const float *depth, const float *th_depth) {
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
            if (!is_anchor) {
                for (int64_t s = slot_off[k]; s < slot_off[k + 1]; ++s) {
                    cv::KeyPoint kp;
                    kp.pt.x = (float)(s - slot_off[k]); kp.pt.y = (float)k; kp.octave = level ? level[s] : 0;
                    F.mvKeysSemantic.push_back(kp);
                    F.mvRight.push_back(right ? right[s] : -1.f);
                    F.mvDepth.push_back(depth ? depth[s] : 1.f);
                }
                F.mThDepth = th_depth ? th_depth[k] : 40.f;
            }
            F.numSemanticKeys = (int)F.mvKeysSemantic.size();
            F.mvpMapPoints.assign(F.mvKeysSemantic.size(), nullptr);
            KeyFrame::nNextId = is_anchor ? (1ul << 20) : (unsigned long)ids[k];
            KF *kf = new KF(F, &map, &db);
            if (is_anchor) anchor = kf; else kfs[k] = kf;
        }
        for (size_t i = 1; i < K; ++i)
            if (!(kfs[order[i - 1]] < kfs[order[i]])) throw std::runtime_error("the arena did not keep the addr order");
        if (K && !(kfs[order[K - 1]] < anchor)) throw std::runtime_error("the anchor is not behind the keyframes");
    }
    void make_points(size_t P) {
        MapPoint::nNextId = 0;
        for (size_t p = 0; p < P; ++p) pts.push_back(new MP(cv::Mat(cv::Mat::zeros(3, 1, CV_32F)), anchor, &map));
        arena_on = false;                                      // from here on the heap: what the routines allocate is the sanitizers' to watch
    }
    std::map<const KeyFrame *, int32_t> kf_index;
    std::map<const MapPoint *, int32_t> pt_index;
    void index_all() {
        for (size_t k = 0; k < kfs.size(); ++k) kf_index[kfs[k]] = (int32_t)k;
        kf_index[anchor] = (int32_t)kfs.size();
        for (size_t p = 0; p < pts.size(); ++p) pt_index[pts[p]] = (int32_t)p;
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
    ~World() {                                                  // the objects lie in the arena; what they hold on the heap goes back
        for (MP *p : pts) p->~MP();
        for (KF *k : kfs) k->~KF();
        if (anchor) anchor->~KF();
        arena_end();
    }
};

struct GraphData {
    int32_t n_kf, n_points;
    std::vector<int64_t> ids, slot_off, first, obs_off;
    std::vector<uint8_t> not_erase, slot_level, bad;
    std::vector<float> th_depth, slot_right, slot_depth;
    std::vector<int32_t> slot_point, found, visible, n_obs, obs_kf, obs_idx;
    explicit GraphData(BlobReader &r) {
        n_kf = r.one<int32_t>(); n_points = r.one<int32_t>();
        if (n_kf < 0 || n_points < 0) throw std::runtime_error("negative count");
        const size_t K = (size_t)n_kf, P = (size_t)n_points;
        ids = r.many<int64_t>(K); not_erase = r.many<uint8_t>(K); th_depth = r.many<float>(K); slot_off = r.many<int64_t>(K + 1);
        const size_t ns = (size_t)slot_off[K];
        slot_point = r.many<int32_t>(ns); slot_level = r.many<uint8_t>(ns); slot_right = r.many<float>(ns); slot_depth = r.many<float>(ns);
        bad = r.many<uint8_t>(P); found = r.many<int32_t>(P); visible = r.many<int32_t>(P); first = r.many<int64_t>(P); n_obs = r.many<int32_t>(P);
        obs_off = r.many<int64_t>(P + 1);
        obs_kf = r.many<int32_t>((size_t)obs_off[P]); obs_idx = r.many<int32_t>((size_t)obs_off[P]);
    }
};

struct Trailer {
    std::vector<int64_t> addr, w_off;
    std::vector<uint8_t> kf_bad, first_connection;
    std::vector<int32_t> parent, w_kf, w_val;
    int32_t links = 0;
    Trailer(BlobReader &r, size_t K) {
        addr = r.many<int64_t>(K); kf_bad = r.many<uint8_t>(K); links = r.one<int32_t>();
        if (links) {
            parent = r.many<int32_t>(K); first_connection = r.many<uint8_t>(K); w_off = r.many<int64_t>(K + 1);
            w_kf = r.many<int32_t>((size_t)w_off[K]); w_val = r.many<int32_t>((size_t)w_off[K]);
        }
        if (r.at != r.buf.size()) throw std::runtime_error("bytes behind the trailer");
    }
};

void build(World &W, const GraphData &d, const Trailer &t, bool anchor_parents) {
    const size_t K = (size_t)d.n_kf, P = (size_t)d.n_points;
    W.make_keyframes(d.ids, t.addr, d.slot_off, d.slot_level.data(), d.slot_right.data(), d.slot_depth.data(), d.th_depth.data());
    W.make_points(P);
    W.index_all();
    for (size_t k = 0; k < K; ++k) {
        KF *kf = W.kfs[k];
        if (kf->mnId != (unsigned long)d.ids[k]) throw std::runtime_error("mnId was not taken from nNextId");
        kf->mbNotErase = d.not_erase[k] != 0;
        kf->mbBad = t.kf_bad[k] != 0;
        for (int64_t s = d.slot_off[k]; s < d.slot_off[k + 1]; ++s)
            if (d.slot_point[(size_t)s] >= 0) kf->AddMapPoint(W.pts.at((size_t)d.slot_point[(size_t)s]), (size_t)(s - d.slot_off[k]));
    }
    for (size_t p = 0; p < P; ++p) {
        MP *mp = W.pts[p];
        mp->mnFirstKFid = (long)d.first[p]; mp->mnFound = d.found[p]; mp->mnVisible = d.visible[p];
        for (int64_t o = d.obs_off[p]; o < d.obs_off[p + 1]; ++o) {
            KF *kf = W.kfs.at((size_t)d.obs_kf[(size_t)o]);
            if ((size_t)d.obs_idx[(size_t)o] >= kf->mvRight.size()) throw std::runtime_error("an observation's idx is no slot of its keyframe");
            mp->AddObservation(kf, (size_t)d.obs_idx[(size_t)o]);
        }
        mp->nObs = d.n_obs[p];
        mp->mbBad = d.bad[p] != 0;
    }
    if (t.links) {
        for (size_t k = 0; k < K; ++k) {
            for (int64_t j = t.w_off[k]; j < t.w_off[k + 1]; ++j) W.kfs[k]->AddConnection(W.kfs.at((size_t)t.w_kf[(size_t)j]), t.w_val[(size_t)j]);
            if (t.parent[k] >= 0) W.kfs[k]->ChangeParent(W.kfs.at((size_t)t.parent[k]));
            else if (anchor_parents) W.kfs[k]->ChangeParent(W.anchor);
            W.kfs[k]->mbFirstConnection = t.first_connection[k] != 0;
        }
    } else if (anchor_parents) {
        for (KF *kf : W.kfs) kf->ChangeParent(W.anchor);
    }
}

struct Out : BlobWriter {
    void words(const std::vector<int32_t> &w) { put(w); }
};

int run_covis(const std::string &mode, const char *in, const char *out) {
    BlobReader r(in);
    const GraphData d(r);
    const size_t K = (size_t)d.n_kf;
    World W;
    std::vector<int32_t> w;
    if (mode == "connections") {
        const int32_t n = r.one<int32_t>();
        const std::vector<int32_t> order = r.many<int32_t>((size_t)n);
        const Trailer t(r, K);
        build(W, d, t, false);
        for (int32_t k : order) W.kfs.at((size_t)k)->UpdateConnections();
        W.dump(w);
    } else if (mode == "kfcull") {
        const int32_t mono = r.one<int32_t>(), n = r.one<int32_t>();
        const std::vector<int32_t> local = r.many<int32_t>((size_t)n);
        const Trailer t(r, K);
        build(W, d, t, true);
        for (int32_t k : local) W.anchor->mvpOrderedConnectedKeyFrames.push_back(W.kfs.at((size_t)k));
        LM lm(&W.map, mono != 0);
        lm.mpCurrentKeyFrame = W.anchor;
        lm.KeyFrameCulling();
        W.dump(w);
        w.push_back((int32_t)W.db.erased.size());
        for (const KeyFrame *kf : W.db.erased) w.push_back(W.ik(kf));
    } else if (mode == "mpcull") {
        const int32_t mono = r.one<int32_t>();
        const int64_t cur = r.one<int64_t>();
        const int32_t n = r.one<int32_t>();
        const std::vector<int32_t> list = r.many<int32_t>((size_t)n);
        const Trailer t(r, K);
        build(W, d, t, false);
        W.anchor->mnId = (unsigned long)cur;
        LM lm(&W.map, mono != 0);
        lm.mpCurrentKeyFrame = W.anchor;
        for (int32_t p : list) lm.mlpRecentAddedMapPoints.push_back(W.pts.at((size_t)p));
        lm.MapPointCulling();
        W.dump(w);
        w.push_back((int32_t)lm.mlpRecentAddedMapPoints.size());
        for (const MapPoint *p : lm.mlpRecentAddedMapPoints) w.push_back(W.ip(p));
    } else if (mode == "chain") {
        const int32_t mono = r.one<int32_t>(), frame_id = r.one<int32_t>(), n = r.one<int32_t>();
        const std::vector<int32_t> slots = r.many<int32_t>((size_t)n);
        const Trailer t(r, K);
        build(W, d, t, false);
        std::vector<KF *> by_id(W.kfs);
        std::stable_sort(by_id.begin(), by_id.end(), [](const KF *a, const KF *b) { return a->mnId < b->mnId; });
        for (KF *kf : by_id) kf->UpdateConnections();
        std::vector<int32_t> part;
        W.dump(part);
        w.push_back((int32_t)part.size()); w.insert(w.end(), part.begin(), part.end());
        LM lm(&W.map, mono != 0);
        lm.mpCurrentKeyFrame = by_id.back();
        lm.KeyFrameCulling();
        part.clear();
        W.dump(part);
        w.push_back((int32_t)part.size()); w.insert(w.end(), part.begin(), part.end());
        w.push_back((int32_t)W.db.erased.size());
        for (const KeyFrame *kf : W.db.erased) w.push_back(W.ik(kf));
        cv::FileStorage::scripted()["ThConfidence"] = 0.5;
        TR tr(&W.map, &W.db);
        tr.mCurrentFrame.mnId = (unsigned long)frame_id;
        tr.mCurrentFrame.numSemanticKeys = n;
        for (int32_t p : slots) tr.mCurrentFrame.mvpMapPoints.push_back(p < 0 ? nullptr : W.pts.at((size_t)p));
        tr.UpdateLocalMap();
        w.push_back((int32_t)tr.mvpLocalKeyFrames.size());
        for (const KeyFrame *kf : tr.mvpLocalKeyFrames) w.push_back(W.ik(kf));
        w.push_back((int32_t)tr.mvpLocalMapPoints.size());
        for (const MapPoint *p : tr.mvpLocalMapPoints) w.push_back(W.ip(p));
        w.push_back(W.ik(tr.mpReferenceKF)); w.push_back(W.ik(tr.mCurrentFrame.mpReferenceKF));
        for (const MapPoint *p : tr.mCurrentFrame.mvpMapPoints) w.push_back(W.ip(p));
        for (const KF *kf : W.kfs) w.push_back((int32_t)kf->mnTrackReferenceForFrame);
        for (const MP *p : W.pts) w.push_back((int32_t)p->mnTrackReferenceForFrame);
    } else {
        throw BlobUsage();
    }
    Out o;
    o.words(w);
    o.save(out);
    return 0;
}

// an array of tests/localmap_cases.arr: i64 n (-1: absent) and the values
template <class T> struct Arr {
    bool present;
    std::vector<T> v;
    explicit Arr(BlobReader &r) {
        const int64_t n = r.one<int64_t>();
        present = n >= 0;
        if (present) v = r.many<T>((size_t)n);
    }
};

int run_localmap(const char *in, const char *out) {
    BlobReader r(in);
    const int32_t n_kf = r.one<int32_t>(), n_points = r.one<int32_t>();
    if (n_kf < 0 || n_points < 0) throw std::runtime_error("negative count");
    const size_t K = (size_t)n_kf, P = (size_t)n_points;
    const Arr<int64_t> obs_off(r); const Arr<int32_t> obs_kf(r); const Arr<uint8_t> point_bad(r), kf_bad(r);
    const Arr<int64_t> slot_off(r); const Arr<int32_t> slot_point(r); const Arr<int64_t> covis_off(r); const Arr<int32_t> covis_kf(r);
    const Arr<int64_t> child_off(r); const Arr<int32_t> child_kf(r), parent(r), kf_order(r);
    int32_t a[3];
    r.get(a, 3);
    const Arr<int32_t> fp(r), kp(r), pp(r), prev(r), bad_kfs(r), bad_points(r);
    if (r.at != r.buf.size()) throw std::runtime_error("bytes behind the call");
    if (a[2] >= 0 || !bad_kfs.v.empty() || !bad_points.v.empty()) throw std::runtime_error("late points and late flags are the adapter's business");

    std::vector<int64_t> ids(K), addr(K);
    for (size_t k = 0; k < K; ++k) { ids[k] = (int64_t)k + 1; addr[k] = (int64_t)k; }
    if (kf_order.present)                                      // kf_order[rank] = keyframe: the keyframes in ascending addr
        for (size_t rank = 0; rank < K; ++rank) addr.at((size_t)kf_order.v.at(rank)) = (int64_t)rank;
    World W;
    W.make_keyframes(ids, addr, slot_off.v, nullptr, nullptr, nullptr, nullptr);
    W.make_points(P);
    W.index_all();
    for (size_t k = 0; k < K; ++k) {
        KF *kf = W.kfs[k];
        kf->mbBad = kf_bad.v.at(k) != 0;
        for (int64_t s = slot_off.v[k]; s < slot_off.v[k + 1]; ++s)
            if (slot_point.v[(size_t)s] >= 0) kf->AddMapPoint(W.pts.at((size_t)slot_point.v[(size_t)s]), (size_t)(s - slot_off.v[k]));
        for (int64_t j = covis_off.v[k]; j < covis_off.v[k + 1]; ++j) kf->mvpOrderedConnectedKeyFrames.push_back(W.kfs.at((size_t)covis_kf.v[(size_t)j]));
        for (int64_t j = child_off.v[k]; j < child_off.v[k + 1]; ++j) kf->mspChildren.insert(W.kfs.at((size_t)child_kf.v[(size_t)j]));
        kf->mpParent = parent.v.at(k) < 0 ? nullptr : W.kfs.at((size_t)parent.v[k]);
    }
    for (size_t p = 0; p < P; ++p) {                            // the tables carry no idx and UpdateLocalMap reads none: 0
        for (int64_t o = obs_off.v[p]; o < obs_off.v[p + 1]; ++o) W.pts[p]->mObservations[W.kfs.at((size_t)obs_kf.v[(size_t)o])] = 0;
        W.pts[p]->mbBad = point_bad.v.at(p) != 0;
    }
    const unsigned long frame_id = (unsigned long)a[0];
    for (int32_t k : kp.v) W.kfs.at((size_t)k)->mnTrackReferenceForFrame = frame_id;
    for (int32_t p : pp.v) W.pts.at((size_t)p)->mnTrackReferenceForFrame = frame_id;

    cv::FileStorage::scripted()["ThConfidence"] = 0.5;         // (the constructor leaves the program over a threshold outside (0, 1))
    TR tr(&W.map, &W.db);
    tr.mCurrentFrame.mnId = frame_id;
    tr.mCurrentFrame.numSemanticKeys = (int)fp.v.size();
    for (int32_t p : fp.v) tr.mCurrentFrame.mvpMapPoints.push_back(p < 0 ? nullptr : W.pts.at((size_t)p));
    for (int32_t k : prev.v) tr.mvpLocalKeyFrames.push_back(W.kfs.at((size_t)k));
    tr.mpReferenceKF = a[1] < 0 ? nullptr : W.kfs.at((size_t)a[1]);
    tr.UpdateLocalMap();

    BlobWriter o;
    const int32_t status = 0;
    const int64_t calls = 1;
    o.put(&status, 1); o.put(&calls, 1);
    std::vector<int32_t> w;
    w.push_back((int32_t)tr.mvpLocalKeyFrames.size());
    for (const KeyFrame *kf : tr.mvpLocalKeyFrames) w.push_back(W.ik(kf));
    w.push_back((int32_t)tr.mvpLocalMapPoints.size());
    for (const MapPoint *p : tr.mvpLocalMapPoints) w.push_back(W.ip(p));
    w.push_back(W.ik(tr.mpReferenceKF)); w.push_back(W.ik(tr.mCurrentFrame.mpReferenceKF));
    for (const MapPoint *p : tr.mCurrentFrame.mvpMapPoints) w.push_back(W.ip(p));
    o.put(w);
    std::vector<int64_t> marks;
    for (const KF *kf : W.kfs) marks.push_back((int64_t)kf->mnTrackReferenceForFrame);
    for (const MP *p : W.pts) marks.push_back((int64_t)p->mnTrackReferenceForFrame);
    o.put(marks);
    o.save(out);
    return 0;
}

int run(int argc, char **argv) {
    if (argc != 4) throw BlobUsage();
    const std::string mode = argv[1];
    if (mode == "localmap") return run_localmap(argv[2], argv[3]);
    return run_covis(mode, argv[2], argv[3]);
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "ref_mapgraph connections|kfcull|mpcull|chain|localmap IN OUT", run); }
