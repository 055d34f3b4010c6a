// localmap_standins.hpp — stand-in SLAM types for tests/localmap_adapter_prog.cpp: KeyFrame, MapPoint and Frame with the members
// sivo_amd/api/orbslam/LocalMapAdapter.h reads and writes, the object graph built from the tables of a test blob (the keyframes are laid out
// so that their pointer order is the tables' kf_order), and the reader of that blob, which tests/localmap_prog.cpp shares.
#pragma once
#include <cstdint>
#include <map>
#include <set>
#include <vector>

#include "../include/sivo_hip.h"
#include "blob_io.hpp"

// an array of a blob: i64 n, then n values; n = -1 stands for a NULL pointer
template <class T>
struct LmArr {
    std::vector<T> v;
    bool null = false;
    explicit LmArr(BlobReader &r) {
        const int64_t n = r.one<int64_t>();
        null = n < 0;
        if (n > 0) v = r.many<T>((size_t)n);
    }
    const T *ptr() const { return null ? nullptr : v.data(); }
};

// i32 n_kf, i32 n_points, then the twelve arrays of SivoLocalMapTables in the struct's order
struct LmBlobTables {
    int32_t n_kf, n_points;
    LmArr<int64_t> obs_off;
    LmArr<int32_t> obs_kf;
    LmArr<uint8_t> point_bad, kf_bad;
    LmArr<int64_t> slot_off;
    LmArr<int32_t> slot_point;
    LmArr<int64_t> covis_off;
    LmArr<int32_t> covis_kf;
    LmArr<int64_t> child_off;
    LmArr<int32_t> child_kf, parent, kf_order;
    explicit LmBlobTables(BlobReader &r)
        : n_kf(r.one<int32_t>()), n_points(r.one<int32_t>()), obs_off(r), obs_kf(r), point_bad(r), kf_bad(r), slot_off(r), slot_point(r),
          covis_off(r), covis_kf(r), child_off(r), child_kf(r), parent(r), kf_order(r) {}
    SivoLocalMapTables table() const {
        SivoLocalMapTables t;
        t.n_kf = n_kf; t.n_points = n_points; t.obs_off = obs_off.ptr(); t.obs_kf = obs_kf.ptr(); t.point_bad = point_bad.ptr();
        t.kf_bad = kf_bad.ptr(); t.slot_off = slot_off.ptr(); t.slot_point = slot_point.ptr(); t.covis_off = covis_off.ptr();
        t.covis_kf = covis_kf.ptr(); t.child_off = child_off.ptr(); t.child_kf = child_kf.ptr(); t.parent = parent.ptr();
        t.kf_order = kf_order.ptr();
        return t;
    }
};

namespace standin {

class KeyFrame;

class MapPoint {
 public:
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    std::map<KeyFrame *, size_t> mObservations;
    bool mbBad = false;
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    bool isBad() { return mbBad; }
};

class KeyFrame {
 public:
    long unsigned int mnId = 0;
    long unsigned int mnTrackReferenceForFrame = 0;
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::set<KeyFrame *> mspChildren;
    KeyFrame *mpParent = nullptr;
    bool mbBad = false;
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::set<KeyFrame *> GetChildren() { return mspChildren; }
    KeyFrame *GetParent() { return mpParent; }
    bool isBad() { return mbBad; }
};

struct Frame {
    long unsigned int mnId = 0;
    int numSemanticKeys = 0;
    std::vector<MapPoint *> mvpMapPoints;
    KeyFrame *mpReferenceKF = nullptr;
};

// The graph of a set of (valid) tables.  kf[k] / point[p] are the objects of table index k / p; the keyframes live in one array in the
// tables' kf_order, so that std::less<KeyFrame *> and the std::set of the children walk them in that order.
struct Graph {
    std::vector<KeyFrame> kfStore;
    std::vector<MapPoint> pointStore;
    std::vector<KeyFrame *> kf;
    std::vector<MapPoint *> point;

    explicit Graph(const SivoLocalMapTables &t) : kfStore((size_t)t.n_kf), pointStore((size_t)t.n_points), kf((size_t)t.n_kf), point((size_t)t.n_points) {
        const size_t K = (size_t)t.n_kf, P = (size_t)t.n_points;
        for (size_t i = 0; i < K; ++i) kf[(size_t)(t.kf_order ? t.kf_order[i] : (int32_t)i)] = &kfStore[i];
        for (size_t p = 0; p < P; ++p) {
            point[p] = &pointStore[p];
            point[p]->mnId = p;
            point[p]->mbBad = t.point_bad[p] != 0;
            for (int64_t o = t.obs_off[p]; o < t.obs_off[p + 1]; ++o) point[p]->mObservations[kf[(size_t)t.obs_kf[o]]] = (size_t)(o - t.obs_off[p]);
        }
        for (size_t k = 0; k < K; ++k) {
            KeyFrame *pKF = kf[k];
            pKF->mnId = k + 1;
            pKF->mbBad = t.kf_bad[k] != 0;
            for (int64_t s = t.slot_off[k]; s < t.slot_off[k + 1]; ++s) pKF->mvpMapPoints.push_back(t.slot_point[s] < 0 ? nullptr : point[(size_t)t.slot_point[s]]);
            for (int64_t c = t.covis_off[k]; c < t.covis_off[k + 1]; ++c) pKF->mvpOrderedConnectedKeyFrames.push_back(kf[(size_t)t.covis_kf[c]]);
            for (int64_t c = t.child_off[k]; c < t.child_off[k + 1]; ++c) pKF->mspChildren.insert(kf[(size_t)t.child_kf[c]]);
            if (t.parent[k] >= 0) pKF->mpParent = kf[(size_t)t.parent[k]];
        }
    }
    int32_t index(const KeyFrame *p) const { return p ? (int32_t)p->mnId - 1 : -1; }
};

}  // namespace standin
