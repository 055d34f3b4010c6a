// Tracking::UpdateLocalMap (reference src/orbslam/Tracking.cc:1087-1235) over the SLAM object graph, on a map that stays on the device:
//     SIVO::LocalMapDevice<KeyFrame, MapPoint> dev;           owns a sivo_localmap_t and the pointer <-> index maps
//     dev.Rebuild(vpAllKFs)                                   gathers the tables of include/sivo_hip.h once and uploads them
//     dev.MarkBad(pKF) / dev.MarkBad(pMP)                     isBad() of one keyframe / point became true since the last Rebuild
//     dev.Touch(pKF) / dev.Touch(pMP) / dev.TouchNeighbourhood(pKF)   the tables of an object changed (or the object is new) ...
//     dev.Sync()                                              ... and ONE sivo_localmap_apply sends the rows of what was touched
//     SIVO::UpdateLocalMap(dev, F, vpLocalKeyFrames, vpLocalMapPoints, pReferenceKF)
//                                                             in place of UpdateLocalKeyFrames(); UpdateLocalPoints(); (:1092-1093)
//     dev.BAWindow(pKF, window)                               the window of Optimizer::LocalBundleAdjustment (Optimizer.cc:496-559,
//                                                             :651-670) from ONE sivo_localmap_ba_window, as pointers
//     dev.KeepAttributes()                                    before Rebuild: the handle also keeps every point's position, normal,
//                                                             distance range, descriptor and Observations() (sivo_localmap_set_points),
//                                                             which SIVO::TrackLocalMapSearch of TrackingAdapter.h needs
//     dev.TouchGeometry(pMP)                                  a point moved or changed its descriptor, its observations did not
// as header-only templates.  UpdateLocalMap maps F.mvpMapPoints to indices, makes ONE call to sivo_localmap_update and writes back as the
// reference does: the cleared slots of the frame (:1139), both vectors, mnTrackReferenceForFrame of every listed keyframe and point
// (:1120, :1171, :1200, :1215, :1225), and pReferenceKF and F.mpReferenceKF where a keyframe had the most votes (:1231-1234).
//
// KeyFrame, MapPoint and Frame are template parameters (SLAM data model, outside this library — SURVEY.md 8).  The members read, all the
// reference's own: KeyFrame: GetMapPointMatches, GetVectorCovisibleKeyFrames (mvpOrderedConnectedKeyFrames; the first ten are used,
// KeyFrame.cc:222-230), GetChildren, GetParent, isBad, mnTrackReferenceForFrame; MapPoint: GetObservations, isBad,
// mnTrackReferenceForFrame; Frame: mnId, numSemanticKeys, mvpMapPoints, mpReferenceKF.  BAWindow reads and writes KeyFrame: mnId,
// mnBALocalForKF, mnBAFixedForKF; MapPoint: mnBALocalForKF, GetIndexInKeyFrame.
//
// kf_order, the order in which the reference's std::map<KeyFrame *, int> walks (:1156), is std::less<KeyFrame *> over the pointers; the
// children are listed as the std::set iterates.  A frame slot whose map point the handle does not know — one created after the last
// Rebuild and never synced — is an error, never skipped: its votes would be missing.
//
// Between two Rebuilds the map is kept current by deltas.  Whoever changes an object records it: Touch(pKF) where a keyframe's slots,
// covisibles, children, parent or flag changed, Touch(pMP) where a point's observations or flag changed, TouchNeighbourhood(pKF) for a
// keyframe together with the points in its slots and its covisibles.  Sync() gathers the rows of the recorded objects only — an unknown
// point in a touched keyframe's slots and an unknown keyframe met as an observer, covisible, child or parent are appended and gathered
// as well — and makes one call.  Indices are stable: an object keeps its index until the next Rebuild, which also compacts.  Whatever
// changed and was not touched is stale until it is touched or the map is rebuilt.  One mutex guards the pointer <-> index maps: Sync runs
// on the local mapper's thread, UpdateLocalMap on the tracking thread.
//
// With KeepAttributes() the handle's attribute store follows the same rules: Rebuild sends every point's attributes, Sync re-sends those
// of every point whose row it sends (touched or appended) in one sivo_localmap_set_points behind the apply, and TouchGeometry(pMP) is for
// the callers that change what the store holds without changing the graph: SetWorldPos, UpdateNormalAndDepth and
// ComputeDistinctiveDescriptors after a bundle adjustment, a loop correction or a refresh.  A point that moved and was not touched is
// stale on the device until it is.  MapPoint members read for it: GetWorldPos, GetNormal, GetMinDistance, GetMaxDistance, GetDescriptor,
// Observations (the getters TrackingAdapter.h asks for).
#ifndef SIVO_AMD_API_LOCALMAPADAPTER_H
#define SIVO_AMD_API_LOCALMAPADAPTER_H

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/sivo_hip.h"

namespace SIVO {
namespace localmap_detail {

inline void check(int rc, const char *what) {
    if (rc == SIVO_ERR_INVALID_ARGUMENT) throw std::invalid_argument(std::string(what) + ": " + sivo_last_error());
    if (rc != SIVO_OK) throw std::runtime_error(std::string(what) + ": " + sivo_last_error());
}

}  // namespace localmap_detail

template <class KeyFrameT, class MapPointT>
class LocalMapDevice {
 public:
    LocalMapDevice() {}
    ~LocalMapDevice() {
        if (mHandle) (void)sivo_localmap_destroy(mHandle);
    }
    LocalMapDevice(const LocalMapDevice &) = delete;
    LocalMapDevice &operator=(const LocalMapDevice &) = delete;

    // The tables of every keyframe of the map, in the vector's order (a keyframe's index is its position), and of every map point one of
    // them holds.  A covisible, child, parent or observer outside the vector is an error.
    void Rebuild(const std::vector<KeyFrameT *> &vpAllKFs) {
        std::lock_guard<std::mutex> lock(mMutex);
        mTouchedKFs.clear(); mTouchedPoints.clear(); mTouchedGeometry.clear();
        mvpKFs = vpAllKFs;
        mKFIndex.clear(); mvpPoints.clear(); mPointIndex.clear();
        const size_t K = mvpKFs.size();
        for (size_t k = 0; k < K; ++k)
            if (!mKFIndex.insert(std::make_pair(mvpKFs[k], (int32_t)k)).second) throw std::invalid_argument("LocalMapDevice::Rebuild: a keyframe is listed twice");
        std::vector<int64_t> slotOff(1, 0), covisOff(1, 0), childOff(1, 0), obsOff(1, 0);
        std::vector<int32_t> slotPoint, covisKf, childKf, parent(K, -1), obsKf, order(K);
        std::vector<uint8_t> kfBad(K, 0), pointBad;
        for (size_t k = 0; k < K; ++k) {
            KeyFrameT *pKF = mvpKFs[k];
            kfBad[k] = pKF->isBad() ? 1 : 0;
            const std::vector<MapPointT *> vpMPs = pKF->GetMapPointMatches();
            for (MapPointT *pMP : vpMPs) {
                if (!pMP) { slotPoint.push_back(-1); continue; }
                auto it = mPointIndex.find(pMP);
                if (it == mPointIndex.end()) {
                    it = mPointIndex.insert(std::make_pair(pMP, (int32_t)mvpPoints.size())).first;
                    mvpPoints.push_back(pMP);
                }
                slotPoint.push_back(it->second);
            }
            slotOff.push_back((int64_t)slotPoint.size());
            const std::vector<KeyFrameT *> vNeighs = pKF->GetVectorCovisibleKeyFrames();
            for (size_t i = 0; i < vNeighs.size() && i < 10; ++i) covisKf.push_back(Known(vNeighs[i], "covisible"));   // (KeyFrame.cc:222-230)
            covisOff.push_back((int64_t)covisKf.size());
            const std::set<KeyFrameT *> spChilds = pKF->GetChildren();
            for (KeyFrameT *pChild : spChilds) childKf.push_back(Known(pChild, "child"));
            childOff.push_back((int64_t)childKf.size());
            if (KeyFrameT *pParent = pKF->GetParent()) parent[k] = Known(pParent, "parent");
            order[k] = (int32_t)k;
        }
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return std::less<KeyFrameT *>()(mvpKFs[(size_t)a], mvpKFs[(size_t)b]); });
        for (MapPointT *pMP : mvpPoints) {
            pointBad.push_back(pMP->isBad() ? 1 : 0);
            const std::map<KeyFrameT *, size_t> observations = pMP->GetObservations();
            for (auto mit = observations.begin(); mit != observations.end(); mit++) obsKf.push_back(Known(mit->first, "observer"));
            obsOff.push_back((int64_t)obsKf.size());
        }
        SivoLocalMapTables t;
        t.n_kf = (int32_t)K; t.n_points = (int32_t)mvpPoints.size();
        t.obs_off = obsOff.data(); t.obs_kf = obsKf.data(); t.point_bad = pointBad.data(); t.kf_bad = kfBad.data();
        t.slot_off = slotOff.data(); t.slot_point = slotPoint.data(); t.covis_off = covisOff.data(); t.covis_kf = covisKf.data();
        t.child_off = childOff.data(); t.child_kf = childKf.data(); t.parent = parent.data(); t.kf_order = order.data();
        if (mHandle) localmap_detail::check(sivo_localmap_replace(mHandle, &t), "LocalMapDevice::Rebuild");
        else localmap_detail::check(sivo_localmap_create(&t, &mHandle), "LocalMapDevice::Rebuild");
        mSlotOff.swap(slotOff);
        if (mReadPoint) {                                              // every row: a replace unsets them all
            std::vector<int32_t> all(mvpPoints.size());
            for (size_t p = 0; p < all.size(); ++p) all[p] = (int32_t)p;
            mSendAttributes(all, "LocalMapDevice::Rebuild");
        }
    }

    // From the next Rebuild on the handle keeps the attributes of every point.  (A member template, so that a MapPoint without the six
    // getters still serves a LocalMapDevice that is never asked to keep them.)
    template <class Unused = void>
    void KeepAttributes() {
        std::lock_guard<std::mutex> lock(mMutex);
        mReadPoint = [](MapPointT *pMP, float *X, float *N, float *range, uint8_t *desc, int32_t *nObs) {
            const auto P = pMP->GetWorldPos();
            const auto Pn = pMP->GetNormal();
            for (int k = 0; k < 3; ++k) { X[k] = P.template at<float>(k, 0); N[k] = Pn.template at<float>(k, 0); }
            range[0] = pMP->GetMinDistance(); range[1] = pMP->GetMaxDistance();
            const auto D = pMP->GetDescriptor();
            std::memcpy(desc, D.ptr(0), 32);
            *nObs = (int32_t)pMP->Observations();
        };
        mSendAttributes = [this](const std::vector<int32_t> &idx, const char *who) { this->template SendAttributesNow<Unused>(idx, who); };
    }
    bool KeepsAttributes() const { return (bool)mReadPoint; }

    void MarkBad(KeyFrameT *pKF) {
        std::lock_guard<std::mutex> lock(mMutex);
        const int32_t k = Known(pKF, "keyframe to mark");
        const uint8_t one = 1;
        localmap_detail::check(sivo_localmap_set_bad(mHandle, 0, nullptr, nullptr, 1, &k, &one), "LocalMapDevice::MarkBad");
    }
    void MarkBad(MapPointT *pMP) {
        std::lock_guard<std::mutex> lock(mMutex);
        const auto it = mPointIndex.find(pMP);
        if (it == mPointIndex.end()) throw std::invalid_argument("LocalMapDevice::MarkBad: the map point was created after the last Rebuild");
        const uint8_t one = 1;
        localmap_detail::check(sivo_localmap_set_bad(mHandle, 1, &it->second, &one, 0, nullptr, nullptr), "LocalMapDevice::MarkBad");
    }

    // An object whose tables changed since the last Rebuild or Sync, or a new one.
    void Touch(KeyFrameT *pKF) {
        std::lock_guard<std::mutex> lock(mMutex);
        if (pKF) mTouchedKFs.insert(pKF);
    }
    void Touch(MapPointT *pMP) {
        std::lock_guard<std::mutex> lock(mMutex);
        if (pMP) mTouchedPoints.insert(pMP);
    }
    // A point whose position, normal, distance range or descriptor changed while its observations did not.
    void TouchGeometry(MapPointT *pMP) {
        std::lock_guard<std::mutex> lock(mMutex);
        if (pMP) mTouchedGeometry.insert(pMP);
    }
    // The keyframe, the points in its slots and its covisibles: what ProcessNewKeyFrame, CreateNewMapPoints and SearchInNeighbors change.
    void TouchNeighbourhood(KeyFrameT *pKF) {
        if (!pKF) return;
        const std::vector<MapPointT *> vpMPs = pKF->GetMapPointMatches();
        const std::vector<KeyFrameT *> vNeighs = pKF->GetVectorCovisibleKeyFrames();
        std::lock_guard<std::mutex> lock(mMutex);
        mTouchedKFs.insert(pKF);
        for (MapPointT *pMP : vpMPs)
            if (pMP) mTouchedPoints.insert(pMP);
        for (KeyFrameT *pN : vNeighs)
            if (pN) mTouchedKFs.insert(pN);
    }

    // The rows of everything touched, and of everything new they lead to, in ONE sivo_localmap_apply; nothing touched: no call.
    void Sync() {
        std::lock_guard<std::mutex> lock(mMutex);
        if (mTouchedKFs.empty() && mTouchedPoints.empty() && mTouchedGeometry.empty()) return;
        if (!mHandle) throw std::invalid_argument("LocalMapDevice::Sync: Rebuild has not run");
        for (MapPointT *pMP : mTouchedGeometry)                         // a point the handle does not know is appended with its row
            if (!mPointIndex.count(pMP)) mTouchedPoints.insert(pMP);
        if (mTouchedKFs.empty() && mTouchedPoints.empty()) {           // geometry alone: no row of the graph changes
            SendTouchedAttributes(std::set<int32_t>());
            mTouchedGeometry.clear();
            return;
        }
        const size_t K0 = mvpKFs.size(), P0 = mvpPoints.size();
        struct KfRow { uint8_t bad; int32_t parent; std::vector<int32_t> slots, covis, children; };
        std::map<int32_t, KfRow> kfRows;                               // by index: the delta lists its rows in increasing order
        std::map<int32_t, std::pair<uint8_t, std::vector<int32_t>>> pointRows;
        std::vector<KeyFrameT *> kfQueue(mTouchedKFs.begin(), mTouchedKFs.end());
        std::vector<MapPointT *> pointQueue(mTouchedPoints.begin(), mTouchedPoints.end());
        auto kfIndex = [&](KeyFrameT *pKF) {                           // an unknown keyframe is appended and gathered as well
            auto it = mKFIndex.find(pKF);
            if (it == mKFIndex.end()) {
                it = mKFIndex.insert(std::make_pair(pKF, (int32_t)mvpKFs.size())).first;
                mvpKFs.push_back(pKF);
                kfQueue.push_back(pKF);
            }
            return it->second;
        };
        auto pointIndex = [&](MapPointT *pMP) {
            auto it = mPointIndex.find(pMP);
            if (it == mPointIndex.end()) {
                it = mPointIndex.insert(std::make_pair(pMP, (int32_t)mvpPoints.size())).first;
                mvpPoints.push_back(pMP);
                pointQueue.push_back(pMP);
            }
            return it->second;
        };
        try {
            while (!kfQueue.empty() || !pointQueue.empty()) {
                if (!kfQueue.empty()) {
                    KeyFrameT *pKF = kfQueue.back();
                    kfQueue.pop_back();
                    const int32_t k = kfIndex(pKF);
                    if (kfRows.count(k)) continue;
                    KfRow &row = kfRows[k];
                    row.bad = pKF->isBad() ? 1 : 0;
                    const std::vector<MapPointT *> vpMPs = pKF->GetMapPointMatches();
                    for (MapPointT *pMP : vpMPs) row.slots.push_back(pMP ? pointIndex(pMP) : -1);
                    const std::vector<KeyFrameT *> vNeighs = pKF->GetVectorCovisibleKeyFrames();
                    for (size_t i = 0; i < vNeighs.size() && i < 10; ++i) row.covis.push_back(kfIndex(vNeighs[i]));      // (KeyFrame.cc:222-230)
                    const std::set<KeyFrameT *> spChilds = pKF->GetChildren();
                    for (KeyFrameT *pChild : spChilds) row.children.push_back(kfIndex(pChild));
                    KeyFrameT *pParent = pKF->GetParent();
                    row.parent = pParent ? kfIndex(pParent) : -1;
                } else {
                    MapPointT *pMP = pointQueue.back();
                    pointQueue.pop_back();
                    const int32_t p = pointIndex(pMP);
                    if (pointRows.count(p)) continue;
                    std::pair<uint8_t, std::vector<int32_t>> &row = pointRows[p];
                    row.first = pMP->isBad() ? 1 : 0;
                    const std::map<KeyFrameT *, size_t> observations = pMP->GetObservations();
                    for (auto mit = observations.begin(); mit != observations.end(); mit++) row.second.push_back(kfIndex(mit->first));
                }
            }
            // (a keyframe or point appended by the lambdas stands in its queue until its row is gathered: every new index is listed)
            std::vector<int32_t> pointIdx, obsKf, kfIdx, parent, slotPoint, covisKf, childKf, order;
            std::vector<int64_t> obsOff(1, 0), slotOff(1, 0), covisOff(1, 0), childOff(1, 0);
            std::vector<uint8_t> pointBad, kfBad;
            for (const auto &e : pointRows) {
                pointIdx.push_back(e.first); pointBad.push_back(e.second.first);
                obsKf.insert(obsKf.end(), e.second.second.begin(), e.second.second.end());
                obsOff.push_back((int64_t)obsKf.size());
            }
            for (const auto &e : kfRows) {
                kfIdx.push_back(e.first); kfBad.push_back(e.second.bad); parent.push_back(e.second.parent);
                slotPoint.insert(slotPoint.end(), e.second.slots.begin(), e.second.slots.end());
                slotOff.push_back((int64_t)slotPoint.size());
                covisKf.insert(covisKf.end(), e.second.covis.begin(), e.second.covis.end());
                covisOff.push_back((int64_t)covisKf.size());
                childKf.insert(childKf.end(), e.second.children.begin(), e.second.children.end());
                childOff.push_back((int64_t)childKf.size());
            }
            for (const auto &e : mKFIndex) order.push_back(e.second);  // the std::map walks in std::less<KeyFrame *>: kf_order
            SivoLocalMapDelta d;
            d.size = (uint32_t)sizeof(SivoLocalMapDelta);
            d.n_kf = (int32_t)mvpKFs.size(); d.n_points = (int32_t)mvpPoints.size();
            d.n_point_rows = (int32_t)pointIdx.size(); d.point_idx = pointIdx.data(); d.point_obs_off = obsOff.data(); d.point_obs_kf = obsKf.data();
            d.point_bad = pointBad.data();
            d.n_kf_rows = (int32_t)kfIdx.size(); d.kf_idx = kfIdx.data(); d.kf_bad = kfBad.data(); d.kf_parent = parent.data();
            d.kf_slot_off = slotOff.data(); d.kf_slot_point = slotPoint.data(); d.kf_covis_off = covisOff.data(); d.kf_covis_kf = covisKf.data();
            d.kf_child_off = childOff.data(); d.kf_child_kf = childKf.data(); d.kf_order = order.data();
            localmap_detail::check(sivo_localmap_apply(mHandle, &d), "LocalMapDevice::Sync");
            std::vector<int64_t> len(mvpKFs.size(), 0);                // mSlotOff follows, in O(keyframes)
            for (size_t k = 0; k < K0; ++k) len[k] = mSlotOff[k + 1] - mSlotOff[k];
            for (const auto &e : kfRows) len[(size_t)e.first] = (int64_t)e.second.slots.size();
            mSlotOff.assign(mvpKFs.size() + 1, 0);
            for (size_t k = 0; k < mvpKFs.size(); ++k) mSlotOff[k + 1] = mSlotOff[k] + len[k];
        } catch (...) {                                                 // the handle is as it was: so are the maps, and the marks stay for a retry
            for (size_t k = K0; k < mvpKFs.size(); ++k) mKFIndex.erase(mvpKFs[k]);
            for (size_t p = P0; p < mvpPoints.size(); ++p) mPointIndex.erase(mvpPoints[p]);
            mvpKFs.resize(K0); mvpPoints.resize(P0);
            throw;
        }
        std::set<int32_t> sent;                                         // the points whose row went up: their attributes follow
        for (const auto &e : pointRows) sent.insert(e.first);
        SendTouchedAttributes(sent);
        mTouchedKFs.clear(); mTouchedPoints.clear(); mTouchedGeometry.clear();
    }

    // What Optimizer::LocalBundleAdjustment has built when it starts to optimise (reference src/orbslam/Optimizer.cc:496-559, :651-670):
    // lLocalKeyFrames, lLocalMapPoints and lFixedKFs in the reference's order — pose index j is localKFs[j], then fixedKFs[j - size] —
    // and for local point i the edges edgeOff[i] .. edgeOff[i + 1]: the pose index of the observing keyframe and mObservations' idx.
    struct Window {
        std::vector<KeyFrameT *> localKFs, fixedKFs;
        std::vector<MapPointT *> localPoints;
        std::vector<int64_t> edgeOff;
        std::vector<int32_t> edgePose;
        std::vector<size_t> edgeIdx;
    };

    // The window of pKF from ONE sivo_localmap_ba_window on the map as the last Rebuild or Sync left it.  The candidates are pKF and its
    // GetVectorCovisibleKeyFrames() in full; no premarks are passed, so the caller keeps pKF->mnId == 0 — the stamp every object starts
    // with — on the host walk.  An edge whose slot the map cannot name (a stale observation, or a point in two slots of a keyframe) is
    // resolved with pMP->GetIndexInKeyFrame(pKFi).  mnBALocalForKF of every candidate (:500, :508) and listed point (:528) and
    // mnBAFixedForKF of every listed fixed keyframe (:553) are written.  pKF or a covisible the handle does not know — touched and not
    // Synced — is an error.
    void BAWindow(KeyFrameT *pKF, Window &w) {
        std::lock_guard<std::mutex> lock(mMutex);                      // the whole call: it sees the map before a Sync or after it
        if (!mHandle) throw std::invalid_argument("LocalMapDevice::BAWindow: Rebuild has not run");
        std::vector<int32_t> cand(1, Known(pKF, "keyframe of the window"));
        const std::vector<KeyFrameT *> vCovisibleKFs = pKF->GetVectorCovisibleKeyFrames();
        for (KeyFrameT *pKFi : vCovisibleKFs) cand.push_back(Known(pKFi, "covisible of the window's keyframe"));
        int64_t sizes[6];
        localmap_detail::check(sivo_localmap_sizes(mHandle, sizes), "LocalMapDevice::BAWindow");
        const size_t K = mvpKFs.size(), pointCap = (size_t)std::min<int64_t>((int64_t)mvpPoints.size(), mSlotOff.back()), edgeCap = (size_t)sizes[2];
        // (the bounds no result exceeds, in buffers that stay: nothing of their size is allocated or cleared per call)
        std::vector<int32_t> &localKf = mWinLocalKf, &fixedKf = mWinFixedKf, &localPoint = mWinLocalPoint, &edgePose = mWinEdgePose, &edgeSlot = mWinEdgeSlot;
        if (localKf.size() < K) { localKf.resize(K); fixedKf.resize(K); }
        if (localPoint.size() < pointCap) localPoint.resize(pointCap);
        if (edgePose.size() < edgeCap) { edgePose.resize(edgeCap); edgeSlot.resize(edgeCap); }
        if (mWinEdgeOff.size() < pointCap + 1) mWinEdgeOff.resize(pointCap + 1);
        int64_t counts[4] = {0, 0, 0, 0};
        localmap_detail::check(sivo_localmap_ba_window(mHandle, (int)cand.size(), cand.data(), 0, nullptr, 0, nullptr, 0, nullptr, (int)K, localKf.data(),
                                                       fixedKf.data(), (int)pointCap, localPoint.data(), mWinEdgeOff.data(), (int64_t)edgeCap,
                                                       edgePose.data(), edgeSlot.data(), counts),
                               "LocalMapDevice::BAWindow");
        const size_t nLocal = (size_t)counts[0], nPoints = (size_t)counts[1], nFixed = (size_t)counts[2], nEdges = (size_t)counts[3];
        w.localKFs.clear(); w.fixedKFs.clear(); w.localPoints.clear();
        for (size_t j = 0; j < nLocal; ++j) w.localKFs.push_back(mvpKFs[(size_t)localKf[j]]);
        for (size_t j = 0; j < nFixed; ++j) w.fixedKFs.push_back(mvpKFs[(size_t)fixedKf[j]]);
        for (size_t i = 0; i < nPoints; ++i) w.localPoints.push_back(mvpPoints[(size_t)localPoint[i]]);
        w.edgeOff.assign(mWinEdgeOff.begin(), mWinEdgeOff.begin() + (std::ptrdiff_t)(nPoints + 1));
        w.edgePose.assign(edgePose.begin(), edgePose.begin() + (std::ptrdiff_t)nEdges);
        w.edgeIdx.assign(nEdges, 0);
        for (size_t i = 0; i < nPoints; ++i)
            for (int64_t e = w.edgeOff[i]; e < w.edgeOff[i + 1]; ++e) {
                if (edgeSlot[(size_t)e] >= 0) { w.edgeIdx[(size_t)e] = (size_t)edgeSlot[(size_t)e]; continue; }
                const size_t j = (size_t)edgePose[(size_t)e];
                const int idx = w.localPoints[i]->GetIndexInKeyFrame(j < nLocal ? w.localKFs[j] : w.fixedKFs[j - nLocal]);
                if (idx < 0) throw std::runtime_error("LocalMapDevice::BAWindow: the device map holds an observation its map point no longer has (touched and not Synced)");
                w.edgeIdx[(size_t)e] = (size_t)idx;
            }
        for (int32_t k : cand) mvpKFs[(size_t)k]->mnBALocalForKF = pKF->mnId;          // (:500, :508)
        for (MapPointT *pMP : w.localPoints) pMP->mnBALocalForKF = pKF->mnId;           // (:528)
        for (KeyFrameT *pKFi : w.fixedKFs) pKFi->mnBAFixedForKF = pKF->mnId;            // (:553)
    }

    // the index of a keyframe the handle knows (the caller holds mMutex or is the only thread)
    int32_t Known(KeyFrameT *pKF, const char *role) const {
        const auto it = mKFIndex.find(pKF);
        if (it == mKFIndex.end()) throw std::invalid_argument(std::string("LocalMapDevice: a ") + role + " is not among the keyframes of the last Rebuild");
        return it->second;
    }

    // the attributes of the listed points (strictly increasing indices) in ONE sivo_localmap_set_points; the caller holds mMutex.  (Reached
    // through mSendAttributes alone, which KeepAttributes() sets: a program that never keeps attributes does not need the entry point.)
    template <class Unused>
    void SendAttributesNow(const std::vector<int32_t> &idx, const char *who) {
        const size_t n = idx.size();
        if (n == 0) return;
        std::vector<float> pos(3 * n), normal(3 * n), lo(n), hi(n);
        std::vector<uint8_t> desc(32 * n);
        std::vector<int32_t> nObs(n);
        for (size_t i = 0; i < n; ++i) {
            float range[2];
            mReadPoint(mvpPoints[(size_t)idx[i]], &pos[3 * i], &normal[3 * i], range, &desc[32 * i], &nObs[i]);
            lo[i] = range[0]; hi[i] = range[1];
        }
        localmap_detail::check(sivo_localmap_set_points(mHandle, (int)n, idx.data(), pos.data(), normal.data(), lo.data(), hi.data(), desc.data(),
                                                        nObs.data()),
                               who);
    }
    void SendTouchedAttributes(std::set<int32_t> idx) {
        if (!mReadPoint) return;
        for (MapPointT *pMP : mTouchedGeometry) idx.insert(mPointIndex.at(pMP));
        mSendAttributes(std::vector<int32_t>(idx.begin(), idx.end()), "LocalMapDevice::Sync");
    }

    sivo_localmap_t mHandle = nullptr;
    std::vector<KeyFrameT *> mvpKFs;
    std::map<KeyFrameT *, int32_t> mKFIndex;
    std::vector<MapPointT *> mvpPoints;
    std::map<MapPointT *, int32_t> mPointIndex;
    std::vector<int64_t> mSlotOff;          // the slot counts: they bound the point list of a call
    std::mutex mMutex;                      // guards the maps above and the sets below
    std::set<KeyFrameT *> mTouchedKFs;
    std::set<MapPointT *> mTouchedPoints, mTouchedGeometry;
    std::function<void(MapPointT *, float *, float *, float *, uint8_t *, int32_t *)> mReadPoint;      // both set by KeepAttributes()
    std::function<void(const std::vector<int32_t> &, const char *)> mSendAttributes;
    std::vector<int32_t> mWinLocalKf, mWinFixedKf, mWinLocalPoint, mWinEdgePose, mWinEdgeSlot;      // BAWindow's output buffers
    std::vector<int64_t> mWinEdgeOff;
};

namespace localmap_detail {

// the arguments and the output buffers of sivo_localmap_update for one frame; the caller holds dev.mMutex
template <class KeyFrameT, class MapPointT, class FrameT>
struct UpdateCall {
    std::vector<int32_t> framePoint, kfMarked, pointMarked, prev, localKf, localPoint;
    std::vector<uint8_t> cleared;
    int32_t voted = 0, nLocalKf = 0, refKf = -1, nLocalPoints = 0;

    // Every keyframe and point of the handle is asked for mnTrackReferenceForFrame == F.mnId, as the reference asks whatever it meets
    // (:1114, :1198, :1213, :1223).
    UpdateCall(LocalMapDevice<KeyFrameT, MapPointT> &dev, FrameT &F, const std::vector<KeyFrameT *> &vpLocalKeyFrames, const char *who) {
        const size_t S = (size_t)F.numSemanticKeys;
        framePoint.assign(S, -1);
        for (size_t i = 0; i < S; ++i) {
            MapPointT *pMP = F.mvpMapPoints[i];
            if (!pMP) continue;
            const auto it = dev.mPointIndex.find(pMP);
            if (it == dev.mPointIndex.end())
                throw std::runtime_error(std::string(who) + ": frame slot " + std::to_string(i) + " holds a map point the device map does not know (created after the last Rebuild)");
            framePoint[i] = it->second;
        }
        for (KeyFrameT *pKF : vpLocalKeyFrames) prev.push_back(dev.Known(pKF, "local keyframe"));
        for (size_t k = 0; k < dev.mvpKFs.size(); ++k)
            if (dev.mvpKFs[k]->mnTrackReferenceForFrame == F.mnId) kfMarked.push_back((int32_t)k);
        for (size_t p = 0; p < dev.mvpPoints.size(); ++p)
            if (dev.mvpPoints[p]->mnTrackReferenceForFrame == F.mnId) pointMarked.push_back((int32_t)p);
        int64_t gPrev = 0;
        for (int32_t k : prev) gPrev += dev.mSlotOff[(size_t)k + 1] - dev.mSlotOff[(size_t)k];
        const size_t pointCap = (size_t)std::min<int64_t>((int64_t)dev.mvpPoints.size(), std::max<int64_t>(dev.mSlotOff.back(), gPrev));
        localKf.resize(dev.mvpKFs.size()); localPoint.resize(pointCap);
        cleared.assign(S, 0);
    }

    // what the reference leaves behind (:1139, :1150-1172, :1200, :1215, :1225, :1231-1234, :1097-1120)
    void WriteBack(LocalMapDevice<KeyFrameT, MapPointT> &dev, FrameT &F, std::vector<KeyFrameT *> &vpLocalKeyFrames,
                   std::vector<MapPointT *> &vpLocalMapPoints, KeyFrameT *&pReferenceKF) const {
        for (size_t i = 0; i < cleared.size(); ++i)
            if (cleared[i]) F.mvpMapPoints[i] = static_cast<MapPointT *>(nullptr);      // (:1139)
        if (voted) {                                                                    // (:1144-1145: else the list stays)
            vpLocalKeyFrames.clear();                                                   // (:1150)
            for (int32_t j = 0; j < nLocalKf; ++j) {
                KeyFrameT *pKF = dev.mvpKFs[(size_t)localKf[(size_t)j]];
                vpLocalKeyFrames.push_back(pKF);
                pKF->mnTrackReferenceForFrame = F.mnId;                                 // (:1171, :1200, :1215, :1225)
            }
            if (refKf >= 0) {                                                           // (:1231-1234)
                pReferenceKF = dev.mvpKFs[(size_t)refKf];
                F.mpReferenceKF = pReferenceKF;
            }
        }
        vpLocalMapPoints.clear();                                                       // (:1097)
        for (int32_t j = 0; j < nLocalPoints; ++j) {
            MapPointT *pMP = dev.mvpPoints[(size_t)localPoint[(size_t)j]];
            vpLocalMapPoints.push_back(pMP);                                            // (:1119)
            pMP->mnTrackReferenceForFrame = F.mnId;                                     // (:1120)
        }
    }
};

}  // namespace localmap_detail

// In place of UpdateLocalKeyFrames(); UpdateLocalPoints(); (Tracking.cc:1092-1093).
template <class KeyFrameT, class MapPointT, class FrameT>
void UpdateLocalMap(LocalMapDevice<KeyFrameT, MapPointT> &dev, FrameT &F, std::vector<KeyFrameT *> &vpLocalKeyFrames,
                    std::vector<MapPointT *> &vpLocalMapPoints, KeyFrameT *&pReferenceKF) {
    std::lock_guard<std::mutex> lock(dev.mMutex);                  // the whole call: it sees the map before a Sync or after it
    if (!dev.mHandle) throw std::invalid_argument("UpdateLocalMap: Rebuild has not run");
    localmap_detail::UpdateCall<KeyFrameT, MapPointT, FrameT> c(dev, F, vpLocalKeyFrames, "UpdateLocalMap");
    localmap_detail::check(sivo_localmap_update(dev.mHandle, (int)c.framePoint.size(), c.framePoint.data(), (int)c.kfMarked.size(), c.kfMarked.data(),
                                                (int)c.pointMarked.size(), c.pointMarked.data(), (int)c.prev.size(), c.prev.data(), &c.voted,
                                                c.cleared.data(), (int)c.localKf.size(), c.localKf.data(), &c.nLocalKf, &c.refKf,
                                                (int)c.localPoint.size(), c.localPoint.data(), &c.nLocalPoints, nullptr),
                           "UpdateLocalMap");
    c.WriteBack(dev, F, vpLocalKeyFrames, vpLocalMapPoints, pReferenceKF);
}

}  // namespace SIVO

#endif
