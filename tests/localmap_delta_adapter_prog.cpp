// localmap_delta_adapter_prog.cpp — LocalMapDevice::Touch / TouchNeighbourhood / Sync of sivo_amd/api/orbslam/LocalMapAdapter.h on stand-in
// SLAM types (localmap_standins.hpp) over the host build of the C ABI (localmap_delta_host_capi.hpp), as a stand-alone program:
// `localmap_delta_adapter_prog script IN OUT` builds the object graph of a blob's tables (at least 9 keyframes and 20 points), Rebuilds a
// device once and then edits the graph as the local mapper does, step by step, with the Touch calls each edit asks for and ONE Sync per
// step.  After each step Tracking's UpdateLocalMap runs twice on the same frame — through the synced device and through a second device
// freshly Rebuilt over the same graph — and everything both leave is compared ON POINTERS: both vectors, pReferenceKF, F.mpReferenceKF,
// the frame's slots and mnTrackReferenceForFrame of every keyframe and point.  tests/test_localmap_delta_host.py reads the verdicts.
//
//   in : tables (localmap_prog.cpp)
//   out: i32 status (1: an exception, then i32 length + its text, and nothing more), then i64 each: whether the frame that holds a
//        just-created point threw before Sync, whether the text was UpdateLocalMap's "created after the last Rebuild", the apply calls an
//        empty Sync made; then per step (insert_keyframe, fuse_point, cull_keyframe, erase_observation, reorder_covisibles): equal, apply
//        calls so far, local keyframes, local map points, keyframes and points the synced device knows
#include <cstdint>
#include <deque>
#include <exception>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "localmap_delta_host_capi.hpp"
#include "localmap_standins.hpp"

#include "LocalMapAdapter.h"

namespace {

using standin::KeyFrame;
using standin::MapPoint;
typedef SIVO::LocalMapDevice<KeyFrame, MapPoint> Device;

struct World {
    std::vector<KeyFrame *> kfs;
    std::vector<MapPoint *> points;
    std::deque<KeyFrame> newKfs;
    std::deque<MapPoint> newPoints;
    std::vector<KeyFrame *> local;             // what the tracker holds between the frames
    KeyFrame *reference = nullptr;
    long unsigned int frameId = 100;
};

struct Left {
    std::vector<KeyFrame *> localKfs;
    std::vector<MapPoint *> localPoints, frame;
    KeyFrame *reference, *frameReference;
    std::vector<long unsigned int> marks;
    bool operator==(const Left &o) const {
        return localKfs == o.localKfs && localPoints == o.localPoints && frame == o.frame && reference == o.reference &&
               frameReference == o.frameReference && marks == o.marks;
    }
};

std::vector<long unsigned int> marks_of(const World &w) {
    std::vector<long unsigned int> m;
    for (KeyFrame *pKF : w.kfs) m.push_back(pKF->mnTrackReferenceForFrame);
    for (MapPoint *pMP : w.points) m.push_back(pMP->mnTrackReferenceForFrame);
    return m;
}

void set_marks(World &w, const std::vector<long unsigned int> &m) {
    size_t i = 0;
    for (KeyFrame *pKF : w.kfs) pKF->mnTrackReferenceForFrame = m[i++];
    for (MapPoint *pMP : w.points) pMP->mnTrackReferenceForFrame = m[i++];
}

// the frame of a step: every third slot of every second keyframe, from the newest keyframe down; all of them points some slot holds
standin::Frame frame_of(const World &w, int step) {
    standin::Frame F;
    F.mnId = w.frameId;
    for (size_t k = w.kfs.size(); k-- > 0;)
        if ((k + (size_t)step) % 2 == 0 || k + 1 == w.kfs.size())
            for (size_t s = 0; s < w.kfs[k]->mvpMapPoints.size(); s += 3) F.mvpMapPoints.push_back(w.kfs[k]->mvpMapPoints[s]);
    F.mvpMapPoints.push_back(nullptr);
    F.numSemanticKeys = (int)F.mvpMapPoints.size();
    return F;
}

Left track(Device &dev, const World &w, standin::Frame F) {
    Left l;
    l.localKfs = w.local;
    l.reference = w.reference;
    SIVO::UpdateLocalMap(dev, F, l.localKfs, l.localPoints, l.reference);
    l.frame = F.mvpMapPoints;
    l.frameReference = F.mpReferenceKF;
    l.marks = marks_of(w);
    return l;
}

// one frame through the synced device and through a device rebuilt from the graph as it stands; the tracker goes on from the result
void compare(Device &dev, World &w, int step, std::vector<int64_t> &out) {
    ++w.frameId;
    const standin::Frame F = frame_of(w, step);
    const std::vector<long unsigned int> before = marks_of(w);
    const Left synced = track(dev, w, F);
    set_marks(w, before);
    Device fresh;
    fresh.Rebuild(w.kfs);
    const Left rebuilt = track(fresh, w, F);
    out.push_back(synced == rebuilt ? 1 : 0);
    out.push_back(localmap_host::applies());
    out.push_back((int64_t)synced.localKfs.size());
    out.push_back((int64_t)synced.localPoints.size());
    out.push_back((int64_t)dev.mvpKFs.size());
    out.push_back((int64_t)dev.mvpPoints.size());
    w.local = synced.localKfs;
    w.reference = synced.reference;
}

void observe(KeyFrame *pKF, MapPoint *pMP) {
    pMP->mObservations[pKF] = pKF->mvpMapPoints.size();
    pKF->mvpMapPoints.push_back(pMP);
}

int run(int argc, char **argv) {
    if (argc != 4 || std::string(argv[1]) != "script") throw BlobUsage();
    BlobReader r(argv[2]);
    BlobWriter wr;
    const LmBlobTables T(r);
    const SivoLocalMapTables t = T.table();
    if (t.n_kf < 9 || t.n_points < 20) throw std::runtime_error("the script needs 9 keyframes and 20 points");
    standin::Graph g(t);
    World w;
    w.kfs = g.kf;
    w.points = g.point;
    int32_t status = 0;
    std::vector<int64_t> out;
    try {
        Device dev;
        dev.Rebuild(w.kfs);
        dev.Sync();                                                     // nothing touched: no call
        const int64_t emptyApplies = localmap_host::applies();

        // 1. a keyframe inserted with new points (ProcessNewKeyFrame, CreateNewMapPoints)
        w.newKfs.emplace_back();
        KeyFrame *pNew = &w.newKfs.back();
        pNew->mnId = w.kfs.size() + 1;
        w.kfs.push_back(pNew);
        for (size_t p = 0; p < 12; p += 2) observe(pNew, w.points[p]);
        pNew->mvpMapPoints.push_back(nullptr);
        for (int i = 0; i < 4; ++i) {
            w.newPoints.emplace_back();
            MapPoint *pMP = &w.newPoints.back();
            pMP->mnId = w.points.size();
            w.points.push_back(pMP);
            observe(pNew, pMP);
            observe(w.kfs[4], pMP);
        }
        pNew->mvpOrderedConnectedKeyFrames = {w.kfs[0], w.kfs[3], w.kfs[5]};
        w.kfs[0]->mvpOrderedConnectedKeyFrames.insert(w.kfs[0]->mvpOrderedConnectedKeyFrames.begin(), pNew);
        pNew->mpParent = w.kfs[2];
        w.kfs[2]->mspChildren.insert(pNew);
        int64_t lateThrew = 0, lateText = 0;
        try {                                                           // the tracker meets a just-created point before the mapper's Sync
            ++w.frameId;
            (void)track(dev, w, frame_of(w, 0));
        } catch (const std::runtime_error &e) {
            lateThrew = 1;
            lateText = std::string(e.what()).find("created after the last Rebuild") != std::string::npos ? 1 : 0;
        }
        out.push_back(lateThrew); out.push_back(lateText); out.push_back(emptyApplies);
        dev.TouchNeighbourhood(pNew);                                   // the keyframe, its points, its covisibles
        dev.Touch(w.kfs[2]);                                            // its parent got a child
        dev.Touch(w.kfs[4]);                                            // holds the new points too
        dev.Sync();
        compare(dev, w, 0, out);

        // 2. a point replaced as ORBmatcher::Fuse -> MapPoint::Replace does: its observers hold the other point now
        MapPoint *pGone = w.points[1], *pStays = w.points[13];
        for (const auto &obs : pGone->mObservations) {
            KeyFrame *pKF = obs.first;
            for (MapPoint *&slot : pKF->mvpMapPoints)
                if (slot == pGone) slot = pStays;
            if (!pStays->mObservations.count(pKF)) pStays->mObservations[pKF] = obs.second;
            dev.Touch(pKF);
        }
        pGone->mObservations.clear();
        pGone->mbBad = true;
        dev.Touch(pGone); dev.Touch(pStays);
        dev.Sync();
        compare(dev, w, 1, out);

        // 3. a keyframe culled (KeyFrame::SetBadFlag): it leaves the covisibility lists and the observations, its children go to its parent
        KeyFrame *pCull = w.kfs[3], *pParent = pCull->mpParent ? pCull->mpParent : w.kfs[0];
        for (KeyFrame *pKF : w.kfs) {
            std::vector<KeyFrame *> &v = pKF->mvpOrderedConnectedKeyFrames;
            for (size_t i = 0; i < v.size();)
                if (v[i] == pCull) { v.erase(v.begin() + (long)i); dev.Touch(pKF); } else ++i;
        }
        for (MapPoint *pMP : pCull->mvpMapPoints)
            if (pMP && pMP->mObservations.erase(pCull)) dev.Touch(pMP);
        for (KeyFrame *pChild : pCull->mspChildren) {
            pChild->mpParent = pParent;
            pParent->mspChildren.insert(pChild);
            dev.Touch(pChild);
        }
        pCull->mspChildren.clear();
        pParent->mspChildren.erase(pCull);
        pCull->mvpOrderedConnectedKeyFrames.clear();
        pCull->mbBad = true;
        dev.Touch(pCull); dev.Touch(pParent);
        dev.Sync();
        compare(dev, w, 2, out);

        // 4. an observation erased (MapPoint::EraseObservation and KeyFrame::EraseMapPointMatch)
        KeyFrame *pKF6 = w.kfs[6];
        for (MapPoint *&slot : pKF6->mvpMapPoints)
            if (slot) {
                slot->mObservations.erase(pKF6);
                dev.Touch(slot);
                slot = nullptr;
                break;
            }
        dev.Touch(pKF6);
        dev.Sync();
        compare(dev, w, 3, out);

        // 5. a covisibility list reordered (KeyFrame::UpdateBestCovisibles)
        std::vector<KeyFrame *> &v = w.kfs[0]->mvpOrderedConnectedKeyFrames;
        std::vector<KeyFrame *> turned(v.rbegin(), v.rend());
        if (turned == v) turned.push_back(w.kfs[7]);
        v = turned;
        dev.Touch(w.kfs[0]);
        dev.Sync();
        compare(dev, w, 4, out);
    } catch (const std::exception &e) {
        status = 1;
        const std::string msg = e.what();
        const int32_t n = (int32_t)msg.size();
        wr.put(&status, 1); wr.put(&n, 1); wr.put(msg.data(), msg.size());
        wr.save(argv[3]);
        return 0;
    }
    wr.put(&status, 1);
    wr.put(out);
    wr.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "localmap_delta_adapter_prog script IN OUT", run); }
