// frustum_prog.cpp — the host build of the frustum cull (sivo_amd/csrc/frustum_math.hpp through tests/frustum_host_capi.hpp) and the C++
// adapter over it (sivo_amd/api/orbslam/TrackingAdapter.h) with stand-in SLAM types; tests/test_pin_frustum.py compares what it writes
// with the reference's Frame::isInFrustum.  No library, no device: the test also builds it with -fsanitize=address,undefined.
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
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbslam/TrackingAdapter.h"
#include "frustum_host_capi.hpp"

template <class T>
static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static void wr(FILE *f, const T *p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

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
    bool read(FILE *in) {
        if (!rd(in, &n, 1) || n < 0 || n > (1 << 24)) return false;
        pos.resize(3 * (size_t)n); normal.resize(3 * (size_t)n); mind.resize((size_t)n); maxd.resize((size_t)n);
        return rd(in, pos.data(), pos.size()) && rd(in, normal.data(), normal.size()) && rd(in, mind.data(), mind.size()) && rd(in, maxd.data(), maxd.size());
    }
    void fill(TMapPoint &p, size_t i) const {
        for (int k = 0; k < 3; ++k) { p.pos.at<float>(k, 0) = pos[3 * i + (size_t)k]; p.normal.at<float>(k, 0) = normal[3 * i + (size_t)k]; }
        p.minDistance = mind[i]; p.maxDistance = maxd[i];
    }
};

static int cull(FILE *in, FILE *out, bool adapter) {
    SivoFrustum f;
    Points P;
    if (!rd(in, &f, 1) || !P.read(in)) return 2;
    const size_t n = (size_t)P.n;
    std::vector<uint8_t> skip(n), status(n, 0);
    if (!rd(in, skip.data(), n)) return 2;
    std::vector<float> px(n, SENTINEL), py(n, SENTINEL), pxr(n, SENTINEL), vc(n, SENTINEL);
    std::vector<int32_t> level(n, -77);
    if (!adapter) {
        int32_t count = -1;
        if (sivo_frustum_cull(&f, (int)n, P.pos.data(), P.normal.data(), P.mind.data(), P.maxd.data(), skip.data(), status.data(), px.data(), py.data(),
                              pxr.data(), vc.data(), level.data(), &count) != SIVO_OK)
            return 3;
        wr(out, status.data(), n); wr(out, px.data(), n); wr(out, py.data(), n); wr(out, pxr.data(), n); wr(out, vc.data(), n); wr(out, level.data(), n);
        wr(out, &count, 1);
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
    wr(out, status.data(), n); wr(out, px.data(), n); wr(out, py.data(), n); wr(out, pxr.data(), n); wr(out, vc.data(), n); wr(out, level.data(), n);
    return 0;
}

static int table(FILE *in, FILE *out) {
    float lsf;
    int32_t nlevels;
    if (!rd(in, &lsf, 1) || !rd(in, &nlevels, 1) || nlevels < 1 || nlevels > 16 || !(lsf > 0.f)) return 2;
    float T[15] = {0};
    sivo::fr_level_table(lsf, nlevels, T);
    wr(out, T, 15);
    for (int k = 0; k < nlevels - 1; ++k) {
        const int32_t lv[2] = {sivo::fr_level_direct(T[k], lsf, nlevels), sivo::fr_level_direct(nextafterf(T[k], INFINITY), lsf, nlevels)};
        wr(out, lv, 2);
    }
    return 0;
}

static int searchlocal(FILE *in, FILE *out) {
    SivoFrustum f;
    float par[2];
    int64_t id, nk;
    if (!rd(in, &f, 1) || !rd(in, par, 2) || !rd(in, &id, 1) || !rd(in, &nk, 1) || nk < 0 || nk > (1 << 20)) return 2;
    TFrame F;
    F.set(f, 1.2f);
    F.mnId = (long unsigned int)id;
    std::vector<SivoKeyPoint> keys((size_t)nk);
    std::vector<int32_t> slot((size_t)nk);
    F.mvRight.resize((size_t)nk);
    F.mDescriptorsSemantic = cv::Mat::zeros((int)(nk > 0 ? nk : 1), 32, CV_8UC1);
    if (!rd(in, keys.data(), keys.size()) || !rd(in, F.mvRight.data(), (size_t)nk) || !rd(in, F.mDescriptorsSemantic.data, 32 * (size_t)nk) ||
        !rd(in, slot.data(), slot.size()))
        return 2;
    for (const SivoKeyPoint &k : keys) F.mvKeysSemantic.push_back(cv::KeyPoint(k.x, k.y, k.size, k.angle, k.response, k.octave, k.class_id));
    Points P;
    if (!P.read(in)) return 2;
    const size_t n = (size_t)P.n;
    std::vector<uint8_t> bad(n), desc(32 * n);
    std::vector<int64_t> seen(n);
    std::vector<int32_t> obs(n);
    int64_t m;
    if (!rd(in, bad.data(), n) || !rd(in, seen.data(), n) || !rd(in, obs.data(), n) || !rd(in, desc.data(), desc.size()) || !rd(in, &m, 1) || m < 0 || m > (1 << 24))
        return 2;
    std::vector<int32_t> local((size_t)m);
    if (!rd(in, local.data(), local.size())) return 2;
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
    wr(out, ret, 2);
    for (const TMapPoint &p : pts) {
        const int32_t vis = p.nVisible, inview = p.mbTrackInView, lvl = p.mnTrackScaleLevel;
        const int64_t s = (int64_t)p.mnLastFrameSeen;
        const float t[4] = {p.mTrackProjX, p.mTrackProjY, p.mTrackProjXR, p.mTrackViewCos};
        wr(out, &vis, 1); wr(out, &s, 1); wr(out, &inview, 1); wr(out, t, 4); wr(out, &lvl, 1);
    }
    for (TMapPoint *p : F.mvpMapPoints) {
        const int32_t s = p ? (int32_t)(p - pts.data()) : -1;
        wr(out, &s, 1);
    }
    SIVO::ORBmatcher::ReleaseDeviceFrames();
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 4) return 1;
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 1;
    int rc = 1;
    try {
        rc = !strcmp(argv[1], "cull") ? cull(in, out, false) : !strcmp(argv[1], "isinfrustum") ? cull(in, out, true)
             : !strcmp(argv[1], "table") ? table(in, out) : !strcmp(argv[1], "searchlocal") ? searchlocal(in, out) : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 5;
    }
    fclose(in);
    return fclose(out) ? 1 : rc;
}
