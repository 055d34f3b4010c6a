// Test program of tests/test_sim3_host.py and tests/test_gpu_sim3.py: Optimizer::OptimizeSim3 (and its gather step) over minimal
// KeyFrame / MapPoint / Sim3 stand-ins.  Reads a scene in text form on stdin, prints hex floats.
//   gather: the pairs optimizer_detail::gather_sim3 builds (index, x1c, x2c, obs1, inv_sigma2_1, obs2, inv_sigma2_2)
//   run:    (-DSIVO_SIM3_ON_DEVICE, linked against libsivo_hip.so) the return value, g2oS12 after the call, the non-null matches
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbslam/Optimizer.h"

struct TKeyFrame;
struct TMapPoint {
    cv::Mat pos = cv::Mat(3, 1, CV_32F);
    bool bad = false;
    int idx2 = -1;                     // GetIndexInKeyFrame(KF2)
    cv::Mat GetWorldPos() const { return pos; }
    bool isBad() const { return bad; }
    int GetIndexInKeyFrame(TKeyFrame *) const { return idx2; }
};
struct TKeyFrame {
    cv::Mat mK = cv::Mat::zeros(3, 3, CV_32F), Tcw = cv::Mat::zeros(4, 4, CV_32F);
    std::vector<cv::KeyPoint> mvKeysSemantic;
    std::vector<float> mvInvLevelSigma2;
    std::vector<TMapPoint *> mvpMapPoints;
    cv::Mat GetRotation() const { cv::Mat R(3, 3, CV_32F); for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R.at<float>(r, c) = Tcw.at<float>(r, c); return R; }
    cv::Mat GetTranslation() const { cv::Mat t(3, 1, CV_32F); for (int r = 0; r < 3; ++r) t.at<float>(r, 0) = Tcw.at<float>(r, 3); return t; }
    std::vector<TMapPoint *> GetMapPointMatches() const { return mvpMapPoints; }
};
struct TQuat {                         // Eigen::Quaterniond as g2o::Sim3::rotation() hands it out
    double c[4] = {0, 0, 0, 1};
    double &x() { return c[0]; } double &y() { return c[1]; } double &z() { return c[2]; } double &w() { return c[3]; }
    double x() const { return c[0]; } double y() const { return c[1]; } double z() const { return c[2]; } double w() const { return c[3]; }
};
struct TVec3 {
    double c[3] = {0, 0, 0};
    double &operator[](int i) { return c[i]; }
    double operator[](int i) const { return c[i]; }
};
struct TSim3 {
    TQuat r; TVec3 t; double s = 1;
    TSim3() {}
    TSim3(const TQuat &r_, const TVec3 &t_, double s_) : r(r_), t(t_), s(s_) {}
    const TQuat &rotation() const { return r; }
    const TVec3 &translation() const { return t; }
    double scale() const { return s; }
};

static double rd() { double v; if (std::scanf("%lf", &v) != 1) std::exit(2); return v; }
static int ri() { return (int)rd(); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    // scene: nkp1 nkp2 npts nmatch | Tcw1 (12) Tcw2 (12) | K1 K2 (fx fy cx cy) | isig (8) | kp1: x y octave mp | kp2: x y octave |
    //        pts: x y z bad idx2 | matches1 (point or -1) | s12 (8) th2 fix_scale
    const int nk1 = ri(), nk2 = ri(), np = ri(), nm = ri();
    TKeyFrame kf[2];
    for (TKeyFrame &k : kf) {
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) k.Tcw.at<float>(r, c) = (float)rd();
        k.Tcw.at<float>(3, 3) = 1.f;
    }
    for (TKeyFrame &k : kf) {
        k.mK.at<float>(0, 0) = (float)rd(); k.mK.at<float>(1, 1) = (float)rd(); k.mK.at<float>(0, 2) = (float)rd(); k.mK.at<float>(1, 2) = (float)rd();
        k.mK.at<float>(2, 2) = 1.f;
    }
    std::vector<float> isig(8);
    for (float &v : isig) v = (float)rd();
    kf[0].mvInvLevelSigma2 = kf[1].mvInvLevelSigma2 = isig;
    std::vector<TMapPoint> pts((size_t)np);
    std::vector<int> mp1((size_t)nk1);
    for (int i = 0; i < nk1; ++i) {
        cv::KeyPoint kp; kp.pt.x = (float)rd(); kp.pt.y = (float)rd(); kp.octave = ri(); mp1[i] = ri();
        kf[0].mvKeysSemantic.push_back(kp);
    }
    for (int i = 0; i < nk2; ++i) {
        cv::KeyPoint kp; kp.pt.x = (float)rd(); kp.pt.y = (float)rd(); kp.octave = ri();
        kf[1].mvKeysSemantic.push_back(kp);
    }
    for (TMapPoint &p : pts) {
        for (int r = 0; r < 3; ++r) p.pos.at<float>(r, 0) = (float)rd();
        p.bad = ri() != 0; p.idx2 = ri();
    }
    for (int i = 0; i < nk1; ++i) kf[0].mvpMapPoints.push_back(mp1[i] >= 0 ? &pts[(size_t)mp1[i]] : nullptr);
    std::vector<TMapPoint *> matches((size_t)nm);
    for (int i = 0; i < nm; ++i) { const int m = ri(); matches[i] = m >= 0 ? &pts[(size_t)m] : nullptr; }
    if (mode == "gather") {
        std::vector<SivoSim3Match> pairs;
        std::vector<size_t> index;
        SIVO::optimizer_detail::gather_sim3(&kf[0], &kf[1], matches, pairs, index);
        for (size_t k = 0; k < pairs.size(); ++k) {
            const SivoSim3Match &m = pairs[k];
            std::printf("%zu %a %a %a %a %a %a %a %a %a %a %a %a\n", index[k], m.x1c[0], m.x1c[1], m.x1c[2], m.x2c[0], m.x2c[1], m.x2c[2],
                        m.obs1[0], m.obs1[1], m.inv_sigma2_1, m.obs2[0], m.obs2[1], m.inv_sigma2_2);
        }
        return 0;
    }
#ifdef SIVO_SIM3_ON_DEVICE
    if (mode == "run") {
        TSim3 S;
        for (int i = 0; i < 4; ++i) S.r.c[i] = rd();
        for (int i = 0; i < 3; ++i) S.t.c[i] = rd();
        S.s = rd();
        const float th2 = (float)rd();
        const bool fix = ri() != 0;
        const int nIn = SIVO::Optimizer::OptimizeSim3(&kf[0], &kf[1], matches, S, th2, fix);
        std::printf("%d\n%a %a %a %a %a %a %a %a\n", nIn, S.r.c[0], S.r.c[1], S.r.c[2], S.r.c[3], S.t.c[0], S.t.c[1], S.t.c[2], S.s);
        for (int i = 0; i < nm; ++i) std::printf("%d ", matches[i] ? 1 : 0);
        std::printf("\n");
        return 0;
    }
#endif
    return 2;
}
