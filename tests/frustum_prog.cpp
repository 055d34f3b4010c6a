// frustum_prog.cpp — the host build of the frustum cull (sivo_amd/csrc/frustum_math.hpp through tests/frustum_host_capi.hpp) and the C++
// adapter over it (sivo_amd/api/orbslam/TrackingAdapter.h) with stand-in SLAM types; tests/test_pin_frustum.py compares what it writes
// with the reference's Frame::isInFrustum.  No library, no device: the test builds it through tests/host_prog.py, plain and under the
// sanitizers.
//   prog cull IN OUT      IN: SivoFrustum, n (i64), pos (3n f32), normal (3n f32), min_dist, max_dist (n f32 each), skip (n bytes).
//                         OUT: status (n bytes), proj_x, proj_y, proj_xr, view_cos (n f32 each), level (n i32), n_in_view (i32); the
//                         outputs start from the sentinels -12345.f / -77, which the entries of a point out of view must keep.
//   prog table IN OUT     IN: log_scale_factor (f32), nlevels (i32).  OUT: T (15 f32), then per k < nlevels - 1 the level of T[k] and of
//                         the next float above it, by the direct expression (2 i32).
//   prog isinfrustum IN OUT   IN as cull.  SIVO::isInFrustum(F, pMP, cos_limit) on a stand-in point per entry without skip.
//                         OUT: mbTrackInView (n bytes), mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos (n f32 each),
//                         mnTrackScaleLevel (n i32), from the same sentinels.
//   prog searchlocal IN OUT   IN: SivoFrustum, th, nnratio (f32), frame id (i64), keys (i64), SivoKeyPoint per key, mvRight (f32 per key),
//                         descriptors (32 bytes per key), the point in each slot (i32 per key, -1 none), points (i64), pos, normal,
//                         min_dist, max_dist as cull, bad (byte per point), mnLastFrameSeen (i64 per point), Observations (i32 per point),
//                         descriptors (32 bytes per point), local points (i64), their indices (i32 each).
//                         OUT: the return value, nToMatch (i32 each), per point nVisible (i32), mnLastFrameSeen (i64), mbTrackInView
//                         (i32), mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos (f32), mnTrackScaleLevel (i32); per key the point in
//                         the slot (i32).
#include <cstring>
#include <string>
#include <vector>

#include "blob_io.hpp"
#include "orbslam/TrackingAdapter.h"
#include "frustum_host_capi.hpp"

static const float SENTINEL = -12345.f;

struct TMapPoint {
    cv::Mat pos = cv::Mat::zeros(3, 1, CV_32F), normal = cv::Mat::zeros(3, 1, CV_32F), desc = cv::Mat::zeros(1, 32, CV_8UC1);
    float minDistance = 0, maxDistance = 0;
    bool bad = false;
    int nObs = 0, nVisible = 0;
    long unsigned int mnLastFrameSeen = 0;
    bool mbTrackInView = false;
    float mTrackProjX = SENTINEL, mTrackProjY = SENTINEL, mTrackProjXR = SENTINEL, mTrackViewCos = SENTINEL;
    int mnTrackScaleLevel = -77;
    bool isBad() const { return bad; }
    void IncreaseVisible(int n = 1) { nVisible += n; }
    int Observations() const { return nObs; }
    cv::Mat GetWorldPos() const { return pos.clone(); }
    cv::Mat GetNormal() const { return normal.clone(); }
    cv::Mat GetDescriptor() const { return desc.clone(); }
    float GetMinDistance() const { return minDistance; }
    float GetMaxDistance() const { return maxDistance; }
};

struct TFrame {
    std::vector<cv::KeyPoint> mvKeysSemantic;
    std::vector<float> mvRight;
    cv::Mat mDescriptorsSemantic = cv::Mat::zeros(1, 32, CV_8UC1);
    std::vector<TMapPoint *> mvpMapPoints;
    cv::Mat mTcw = cv::Mat::eye(4, 4, CV_32F);
    float fx = 1, fy = 1, cx = 0, cy = 0, mbf = 0, mnMinX = 0, mnMaxX = 1, mnMinY = 0, mnMaxY = 1, mfLogScaleFactor = 1;
    int mnScaleLevels = 1;
    std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
    long unsigned int mnId = 0;
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

struct Points {
    int64_t n = 0;
    std::vector<float> pos, normal, mind, maxd;
    bool read(BlobReader &in) {
        n = in.one<int64_t>();
        if (n < 0 || n > (1 << 24)) return false;
        pos = in.many<float>(3 * (size_t)n); normal = in.many<float>(3 * (size_t)n); mind = in.many<float>((size_t)n); maxd = in.many<float>((size_t)n);
        return true;
    }
    void fill(TMapPoint &p, size_t i) const {
        for (int k = 0; k < 3; ++k) { p.pos.at<float>(k, 0) = pos[3 * i + (size_t)k]; p.normal.at<float>(k, 0) = normal[3 * i + (size_t)k]; }
        p.minDistance = mind[i]; p.maxDistance = maxd[i];
    }
};

static int cull(BlobReader &in, BlobWriter &out, bool adapter) {
    const SivoFrustum f = in.one<SivoFrustum>();
    Points P;
    if (!P.read(in)) return 2;
    const size_t n = (size_t)P.n;
    const std::vector<uint8_t> skip = in.many<uint8_t>(n);
    std::vector<uint8_t> status(n, 0);
    std::vector<float> px(n, SENTINEL), py(n, SENTINEL), pxr(n, SENTINEL), vc(n, SENTINEL);
    std::vector<int32_t> level(n, -77);
    if (!adapter) {
        int32_t count = -1;
        if (sivo_frustum_cull(&f, (int)n, P.pos.data(), P.normal.data(), P.mind.data(), P.maxd.data(), skip.data(), status.data(), px.data(), py.data(),
                              pxr.data(), vc.data(), level.data(), &count) != SIVO_OK)
            return 3;
        out.put(status); out.put(px); out.put(py); out.put(pxr); out.put(vc); out.put(level);
        out.put(&count, 1);
        return 0;
    }
    TFrame F;
    F.set(f, 1.2f);
    for (size_t i = 0; i < n; ++i) {
        TMapPoint p;
        P.fill(p, i);
        if (!skip[i]) {
            const bool in = SIVO::isInFrustum(F, &p, f.cos_limit);
            if (in != p.mbTrackInView) return 4;
        }
        status[i] = p.mbTrackInView;
        px[i] = p.mTrackProjX; py[i] = p.mTrackProjY; pxr[i] = p.mTrackProjXR; vc[i] = p.mTrackViewCos; level[i] = p.mnTrackScaleLevel;
    }
    out.put(status); out.put(px); out.put(py); out.put(pxr); out.put(vc); out.put(level);
    return 0;
}

static int table(BlobReader &in, BlobWriter &out) {
    const float lsf = in.one<float>();
    const int32_t nlevels = in.one<int32_t>();
    if (nlevels < 1 || nlevels > 16 || !(lsf > 0.f)) return 2;
    float T[15] = {0};
    sivo::fr_level_table(lsf, nlevels, T);
    out.put(T, 15);
    for (int k = 0; k < nlevels - 1; ++k) {
        const int32_t lv[2] = {sivo::fr_level_direct(T[k], lsf, nlevels), sivo::fr_level_direct(nextafterf(T[k], INFINITY), lsf, nlevels)};
        out.put(lv, 2);
    }
    return 0;
}

static int searchlocal(BlobReader &in, BlobWriter &out) {
    const SivoFrustum f = in.one<SivoFrustum>();
    float par[2];
    in.get(par, 2);
    const int64_t id = in.one<int64_t>(), nk = in.one<int64_t>();
    if (nk < 0 || nk > (1 << 20)) return 2;
    TFrame F;
    F.set(f, 1.2f);
    F.mnId = (long unsigned int)id;
    const std::vector<SivoKeyPoint> keys = in.many<SivoKeyPoint>((size_t)nk);
    F.mvRight = in.many<float>((size_t)nk);
    F.mDescriptorsSemantic = cv::Mat::zeros((int)(nk > 0 ? nk : 1), 32, CV_8UC1);
    in.get(F.mDescriptorsSemantic.data, 32 * (size_t)nk);
    const std::vector<int32_t> slot = in.many<int32_t>((size_t)nk);
    for (const SivoKeyPoint &k : keys) F.mvKeysSemantic.push_back(cv::KeyPoint(k.x, k.y, k.size, k.angle, k.response, k.octave, k.class_id));
    Points P;
    if (!P.read(in)) return 2;
    const size_t n = (size_t)P.n;
    const std::vector<uint8_t> bad = in.many<uint8_t>(n);
    const std::vector<int64_t> seen = in.many<int64_t>(n);
    const std::vector<int32_t> obs = in.many<int32_t>(n);
    const std::vector<uint8_t> desc = in.many<uint8_t>(32 * n);
    const int64_t m = in.one<int64_t>();
    if (m < 0 || m > (1 << 24)) return 2;
    const std::vector<int32_t> local = in.many<int32_t>((size_t)m);
    std::vector<TMapPoint> pts(n);
    for (size_t i = 0; i < n; ++i) {
        P.fill(pts[i], i);
        pts[i].bad = bad[i] != 0; pts[i].mnLastFrameSeen = (long unsigned int)seen[i]; pts[i].nObs = obs[i];
        std::memcpy(pts[i].desc.data, &desc[32 * i], 32);
    }
    for (int32_t s : slot) {
        if (s >= (int32_t)n) return 2;
        F.mvpMapPoints.push_back(s < 0 ? nullptr : &pts[(size_t)s]);
    }
    std::vector<TMapPoint *> vpLocal;
    for (int32_t i : local) {
        if (i < 0 || i >= (int32_t)n) return 2;
        vpLocal.push_back(&pts[(size_t)i]);
    }
    int32_t ret[2] = {0, -1};
    ret[0] = SIVO::SearchLocalPoints(F, vpLocal, par[0], par[1], &ret[1]);
    out.put(ret, 2);
    for (const TMapPoint &p : pts) {
        const int32_t vis = p.nVisible, inview = p.mbTrackInView, lvl = p.mnTrackScaleLevel;
        const int64_t s = (int64_t)p.mnLastFrameSeen;
        const float t[4] = {p.mTrackProjX, p.mTrackProjY, p.mTrackProjXR, p.mTrackViewCos};
        out.put(&vis, 1); out.put(&s, 1); out.put(&inview, 1); out.put(t, 4); out.put(&lvl, 1);
    }
    for (TMapPoint *p : F.mvpMapPoints) {
        const int32_t s = p ? (int32_t)(p - pts.data()) : -1;
        out.put(&s, 1);
    }
    SIVO::ORBmatcher::ReleaseDeviceFrames();
    return 0;
}

// exit codes beside blob_main's: 2 a count out of range, 3 the cull's return code, 4 isInFrustum and mbTrackInView disagree
static int run(int argc, char **argv) {
    if (argc != 4) throw BlobUsage();
    const std::string mode = argv[1];
    BlobReader in(argv[2]);
    BlobWriter out;
    const int rc = mode == "cull" ? cull(in, out, false) : mode == "isinfrustum" ? cull(in, out, true) : mode == "table" ? table(in, out)
                   : mode == "searchlocal" ? searchlocal(in, out) : throw BlobUsage();
    out.save(argv[3]);
    return rc;
}

int main(int argc, char **argv) { return blob_main(argc, argv, "frustum_prog cull|isinfrustum|table|searchlocal IN OUT", run); }
