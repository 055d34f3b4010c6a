// localmap_track_adapter_prog.cpp — SIVO::TrackLocalMapSearch (sivo_amd/api/orbslam/TrackingAdapter.h) against the pair it replaces,
// SIVO::UpdateLocalMap + SIVO::SearchLocalPoints, on two copies of ONE stand-in object graph over the host build of the entry points
// (tests/localmap_track_host_capi.hpp): copy A runs the pair, copy B the new call, over a script of frames whose slots carry the points
// the frame before ended with.  After every step every field of the frame, every keyframe and every point of both copies is written;
// tests/test_localmap_track_host.py asserts that the two dumps are the same bytes.  No library, no device: plain and under the sanitizers.
//
//   prog run IN OUT    IN: i32 touch_geometry (0: a moved point is NOT reported to copy B's device map), tables (as tests/localmap_prog.cpp),
//                      per point pos, normal (3 f32 each), min_dist, max_dist (f32), Observations() (i32), descriptor (32 bytes);
//                      SivoFrustum, f32 th, nnratio; i64 keys, SivoKeyPoint per key, mvRight f32 per key, descriptors 32 bytes per key;
//                      i64 a frame id and arrays of keyframes and points (i32) whose mnTrackReferenceForFrame holds it from the start;
//                      i32 steps; per step: i64 frame id, arrays slot i32 (per key: the point, -1 none, -2 the point the frame before
//                      ended with), seen i32 (mnLastFrameSeen = the frame's id before the call), bad i32 (isBad() from now on, MarkBad),
//                      moved i32 and their new positions f32 (3 each).
//                      OUT: per step and copy (A, then B): i32 return value, nToMatch, calls of sivo_localmap_update and of
//                      sivo_localmap_search_local_points so far, mpReferenceKF and F.mpReferenceKF as indices; the frame's slots (i32 per
//                      key); mvpLocalKeyFrames and mvpLocalMapPoints (i32 count, then indices); mnTrackReferenceForFrame (i64 per
//                      keyframe); per point nVisible (i32), mnLastFrameSeen, mnTrackReferenceForFrame (i64), mbTrackInView (i32),
//                      mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos (f32), mnTrackScaleLevel (i32).
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "orbslam/TrackingAdapter.h"
#include "localmap_track_host_capi.hpp"
#include "localmap_standins.hpp"

namespace {

const float SENTINEL = -12345.f;
struct TKeyFrame;

struct TPoint {
    long unsigned int mnId = 0, mnTrackReferenceForFrame = 0, mnLastFrameSeen = 0;
    std::map<TKeyFrame *, size_t> mObservations;
    cv::Mat pos = cv::Mat::zeros(3, 1, CV_32F), normal = cv::Mat::zeros(3, 1, CV_32F), desc = cv::Mat::zeros(1, 32, CV_8UC1);
    float minDistance = 0, maxDistance = 0;
    bool bad = false, mbTrackInView = false;
    int nObs = 0, nVisible = 0, mnTrackScaleLevel = -77;
    float mTrackProjX = SENTINEL, mTrackProjY = SENTINEL, mTrackProjXR = SENTINEL, mTrackViewCos = SENTINEL;
    std::map<TKeyFrame *, size_t> GetObservations() { return mObservations; }
    bool isBad() const { return bad; }
    void IncreaseVisible(int n = 1) { nVisible += n; }
    int Observations() const { return nObs; }
    cv::Mat GetWorldPos() const { return pos.clone(); }
    cv::Mat GetNormal() const { return normal.clone(); }
    cv::Mat GetDescriptor() const { return desc.clone(); }
    float GetMinDistance() const { return minDistance; }
    float GetMaxDistance() const { return maxDistance; }
};

struct TKeyFrame {
    long unsigned int mnId = 0, mnTrackReferenceForFrame = 0;
    std::vector<TPoint *> mvpMapPoints;
    std::vector<TKeyFrame *> mvpOrderedConnectedKeyFrames;
    std::set<TKeyFrame *> mspChildren;
    TKeyFrame *mpParent = nullptr;
    bool mbBad = false;
    std::vector<TPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<TKeyFrame *> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    std::set<TKeyFrame *> GetChildren() { return mspChildren; }
    TKeyFrame *GetParent() { return mpParent; }
    bool isBad() { return mbBad; }
};

struct TFrame {
    std::vector<cv::KeyPoint> mvKeysSemantic;
    std::vector<float> mvRight;
    cv::Mat mDescriptorsSemantic = cv::Mat::zeros(1, 32, CV_8UC1);
    std::vector<TPoint *> mvpMapPoints;
    cv::Mat mTcw = cv::Mat::eye(4, 4, CV_32F);
    float fx = 1, fy = 1, cx = 0, cy = 0, mbf = 0, mnMinX = 0, mnMaxX = 1, mnMinY = 0, mnMaxY = 1, mfLogScaleFactor = 1;
    int mnScaleLevels = 1, numSemanticKeys = 0;
    std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    long unsigned int mnId = 0;
    TKeyFrame *mpReferenceKF = nullptr;
    void set(const SivoFrustum &f, float scaleFactor) {
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) mTcw.at<float>(r, c) = f.Rcw[3 * r + c];
            mTcw.at<float>(r, 3) = f.tcw[r];
        }
        fx = f.fx; fy = f.fy; cx = f.cx; cy = f.cy; mbf = f.bf;
        mnMinX = f.min_x; mnMaxX = f.max_x; mnMinY = f.min_y; mnMaxY = f.max_y;
        mfLogScaleFactor = f.log_scale_factor; mnScaleLevels = f.nlevels;
        mvScaleFactors.assign((size_t)f.nlevels, 1.0f); mvLevelSigma2.assign((size_t)f.nlevels, 1.0f); mvInvLevelSigma2.assign((size_t)f.nlevels, 1.0f);
        for (int i = 1; i < f.nlevels; ++i) {                      // ORBextractor.cc: mvScaleFactor[i] = mvScaleFactor[i - 1] * scaleFactor
            mvScaleFactors[(size_t)i] = mvScaleFactors[(size_t)i - 1] * scaleFactor;
            mvLevelSigma2[(size_t)i] = mvScaleFactors[(size_t)i] * mvScaleFactors[(size_t)i];
            mvInvLevelSigma2[(size_t)i] = 1.0f / mvLevelSigma2[(size_t)i];
        }
    }
};

// one copy of the graph: the keyframes in one array in the tables' kf_order, so that std::less<TKeyFrame *> walks them in that order
struct Copy {
    std::vector<TKeyFrame> kfStore;
    std::vector<TPoint> pointStore;
    std::vector<TKeyFrame *> kf;
    SIVO::LocalMapDevice<TKeyFrame, TPoint> dev;
    std::vector<TKeyFrame *> localKFs;
    std::vector<TPoint *> localPoints;
    TKeyFrame *reference = nullptr;
    std::vector<TPoint *> carried;             // the slots the frame before ended with

    Copy(const SivoLocalMapTables &t, const std::vector<float> &pos, const std::vector<float> &normal, const std::vector<float> &lo,
         const std::vector<float> &hi, const std::vector<int32_t> &obs, const std::vector<uint8_t> &desc)
        : kfStore((size_t)t.n_kf), pointStore((size_t)t.n_points), kf((size_t)t.n_kf) {
        const size_t K = (size_t)t.n_kf, P = (size_t)t.n_points;
        for (size_t i = 0; i < K; ++i) kf[(size_t)(t.kf_order ? t.kf_order[i] : (int32_t)i)] = &kfStore[i];
        for (size_t p = 0; p < P; ++p) {
            TPoint &x = pointStore[p];
            x.mnId = p; x.bad = t.point_bad[p] != 0;
            for (int64_t o = t.obs_off[p]; o < t.obs_off[p + 1]; ++o) x.mObservations[kf[(size_t)t.obs_kf[o]]] = (size_t)(o - t.obs_off[p]);
            for (int k = 0; k < 3; ++k) { x.pos.at<float>(k, 0) = pos[3 * p + (size_t)k]; x.normal.at<float>(k, 0) = normal[3 * p + (size_t)k]; }
            x.minDistance = lo[p]; x.maxDistance = hi[p]; x.nObs = obs[p];
            std::memcpy(x.desc.data, &desc[32 * p], 32);
        }
        for (size_t k = 0; k < K; ++k) {
            TKeyFrame *pKF = kf[k];
            pKF->mnId = k + 1; pKF->mbBad = t.kf_bad[k] != 0;
            for (int64_t s = t.slot_off[k]; s < t.slot_off[k + 1]; ++s) pKF->mvpMapPoints.push_back(t.slot_point[s] < 0 ? nullptr : &pointStore[(size_t)t.slot_point[s]]);
            for (int64_t c = t.covis_off[k]; c < t.covis_off[k + 1]; ++c) pKF->mvpOrderedConnectedKeyFrames.push_back(kf[(size_t)t.covis_kf[c]]);
            for (int64_t c = t.child_off[k]; c < t.child_off[k + 1]; ++c) pKF->mspChildren.insert(kf[(size_t)t.child_kf[c]]);
            if (t.parent[k] >= 0) pKF->mpParent = kf[(size_t)t.parent[k]];
        }
    }
    int32_t index(const TKeyFrame *p) const { return p ? (int32_t)p->mnId - 1 : -1; }
    int32_t index(const TPoint *p) const { return p ? (int32_t)p->mnId : -1; }
};

int run(int argc, char **argv) {
    if (argc != 4 || std::string(argv[1]) != "run") throw BlobUsage();
    BlobReader r(argv[2]);
    BlobWriter w;
    const int32_t touch = r.one<int32_t>();
    const LmBlobTables T(r);
    const SivoLocalMapTables t = T.table();
    if (sivo::lm_check_tables(&t)) throw std::runtime_error("the tables are not valid");
    const size_t P = (size_t)t.n_points;
    const std::vector<float> pos = r.many<float>(3 * P), normal = r.many<float>(3 * P), lo = r.many<float>(P), hi = r.many<float>(P);
    const std::vector<int32_t> obs = r.many<int32_t>(P);
    const std::vector<uint8_t> desc = r.many<uint8_t>(32 * P);
    const SivoFrustum f = r.one<SivoFrustum>();
    const float th = r.one<float>(), nn = r.one<float>();
    const int64_t nk = r.one<int64_t>();
    const std::vector<SivoKeyPoint> keys = r.many<SivoKeyPoint>((size_t)nk);
    const std::vector<float> right = r.many<float>((size_t)nk);
    const std::vector<uint8_t> kdesc = r.many<uint8_t>(32 * (size_t)nk);
    Copy A(t, pos, normal, lo, hi, obs, desc), B(t, pos, normal, lo, hi, obs, desc);
    Copy *copies[2] = {&A, &B};
    const int64_t marked = r.one<int64_t>();
    const LmArr<int32_t> markedKf(r), markedPoint(r);
    for (Copy *c : copies) {
        for (int32_t k : markedKf.v) c->kf[(size_t)k]->mnTrackReferenceForFrame = (long unsigned int)marked;
        for (int32_t p : markedPoint.v) c->pointStore[(size_t)p].mnTrackReferenceForFrame = (long unsigned int)marked;
    }
    A.dev.Rebuild(A.kf);
    B.dev.KeepAttributes();
    B.dev.Rebuild(B.kf);
    const int32_t steps = r.one<int32_t>();
    for (int32_t s = 0; s < steps; ++s) {
        const int64_t id = r.one<int64_t>();
        const LmArr<int32_t> slot(r), seen(r), bad(r), moved(r);
        const std::vector<float> to = r.many<float>(3 * moved.v.size());
        for (int which = 0; which < 2; ++which) {
            Copy &c = *copies[which];
            for (int32_t p : bad.v) {
                c.pointStore[(size_t)p].bad = true;
                c.dev.MarkBad(&c.pointStore[(size_t)p]);
            }
            for (size_t i = 0; i < moved.v.size(); ++i) {
                TPoint &x = c.pointStore[(size_t)moved.v[i]];
                for (int k = 0; k < 3; ++k) x.pos.at<float>(k, 0) = to[3 * i + (size_t)k];       // SetWorldPos
                if (which == 1 && touch) c.dev.TouchGeometry(&x);
            }
            c.dev.Sync();
            TFrame F;
            F.set(f, 1.2f);
            F.mnId = (long unsigned int)id;
            for (const SivoKeyPoint &k : keys) F.mvKeysSemantic.push_back(cv::KeyPoint(k.x, k.y, k.size, k.angle, k.response, k.octave, k.class_id));
            F.mvRight = right;
            F.mDescriptorsSemantic = cv::Mat::zeros((int)(nk > 0 ? nk : 1), 32, CV_8UC1);
            std::memcpy(F.mDescriptorsSemantic.data, kdesc.data(), kdesc.size());
            F.numSemanticKeys = (int)nk;
            for (size_t k = 0; k < (size_t)nk; ++k) {
                const int32_t p = slot.v[k];
                F.mvpMapPoints.push_back(p == -2 ? (k < c.carried.size() ? c.carried[k] : nullptr) : p < 0 ? nullptr : &c.pointStore[(size_t)p]);
            }
            for (int32_t p : seen.v) c.pointStore[(size_t)p].mnLastFrameSeen = (long unsigned int)id;
            int32_t ret[2] = {0, -1};
            if (which == 0) {
                SIVO::UpdateLocalMap(c.dev, F, c.localKFs, c.localPoints, c.reference);
                ret[0] = SIVO::SearchLocalPoints(F, c.localPoints, th, nn, &ret[1]);
            } else {
                ret[0] = SIVO::TrackLocalMapSearch(c.dev, F, c.localKFs, c.localPoints, c.reference, th, nn, &ret[1]);
            }
            c.carried = F.mvpMapPoints;
            SIVO::ORBmatcher::ReleaseDeviceFrames();
            w.put(ret, 2);
            const int32_t calls[4] = {(int32_t)localmap_host::calls(), (int32_t)localmap_track_host::searches(), c.index(c.reference), c.index(F.mpReferenceKF)};
            w.put(calls, 4);
            for (TPoint *p : F.mvpMapPoints) { const int32_t i = c.index(p); w.put(&i, 1); }
            int32_t n = (int32_t)c.localKFs.size();
            w.put(&n, 1);
            for (TKeyFrame *p : c.localKFs) { const int32_t i = c.index(p); w.put(&i, 1); }
            n = (int32_t)c.localPoints.size();
            w.put(&n, 1);
            for (TPoint *p : c.localPoints) { const int32_t i = c.index(p); w.put(&i, 1); }
            for (TKeyFrame *p : c.kf) { const int64_t m = (int64_t)p->mnTrackReferenceForFrame; w.put(&m, 1); }
            for (const TPoint &p : c.pointStore) {
                const int32_t vis = p.nVisible, inview = p.mbTrackInView, lvl = p.mnTrackScaleLevel;
                const int64_t marks[2] = {(int64_t)p.mnLastFrameSeen, (int64_t)p.mnTrackReferenceForFrame};
                const float tr[4] = {p.mTrackProjX, p.mTrackProjY, p.mTrackProjXR, p.mTrackViewCos};
                w.put(&vis, 1); w.put(marks, 2); w.put(&inview, 1); w.put(tr, 4); w.put(&lvl, 1);
            }
        }
    }
    w.save(argv[3]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) { return blob_main(argc, argv, "localmap_track_adapter_prog run IN OUT", run); }
