// Driver of the reference's OWN Sim3Solver (src/orbslam/Sim3Solver.cc, compiled untouched into oracle/_ref/ref_sim3solver.o with
// its protected members made reachable) for tests/test_pin_solvers.py.  Text on stdin, hex floats out.
//   core:   `n fix_scale K1[4] K2[4]`, n pairs (x1c[3] x2c[3] max_err1 max_err2), `ntriples`, the triples.  The members the
//           constructor would fill are set from the pairs (the projections by the reference's FromCameraToImage); per triple the
//           sample is copied as iterate does, then the reference's ComputeSim3 / CheckInliers.  Printed: count, mR12i (9),
//           mt12i (3), ms12i, the upper three rows of mT12i and of mT21i, the inlier words
//   gather: candidates in the text form of tests/sim3_ransac_restatement.py scene_text; what the constructor computed:
//           candidate, mvnIndices1, mvX3Dc1, mvX3Dc2, mvnMaxError1 / 2 (as the floats the comparison converts them to), mvP1im1, mvP2im2
//   run:    per candidate `probability minInliers maxIterations ndraws draws...` follow the scene; the round-robin of
//           LoopClosing.cc:294-313 until every candidate said bNoMore or was called argv[2] times, iterate(argv[3], default 5) per call
//           (0: find()); every call is printed as tests/sim3_ransac_prog.cpp prints it.  DUtils::Random::RandomInt reads the draws of the
//           candidate being called.  Further arguments: "shared" (every candidate draws from the first one's list: one stream for all, as
//           the reference's global one), "keep" (a candidate is called again after bNoMore, until argv[2] calls)
//   params: lines `N probability minInliers maxIterations`: mRansacMaxIts after SetRansacParameters on a solver of N pairs
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "include/orbslam/Sim3Solver.h"
#include "dependencies/DBoW2/DUtils/Random.h"

using SIVO::KeyFrame;
using SIVO::MapPoint;
using SIVO::Sim3Solver;

static double rd() { double v; if (std::scanf("%lf", &v) != 1) std::exit(2); return v; }
static int ri() { return (int)rd(); }

struct Candidate {
    KeyFrame kf[2];
    std::vector<MapPoint> pts;
    std::vector<MapPoint *> matches;
    bool fix = true;
    std::unique_ptr<Sim3Solver> solver;
    DUtils::Random::Script script;
};

static void read_K(KeyFrame &k) {
    k.mK.at<float>(0, 0) = (float)rd(); k.mK.at<float>(1, 1) = (float)rd(); k.mK.at<float>(0, 2) = (float)rd(); k.mK.at<float>(1, 2) = (float)rd();
    k.mK.at<float>(2, 2) = 1.f;
}

static void read_candidate(Candidate &c) {
    const int nk1 = ri(), nk2 = ri(), np = ri(), nm = ri();
    c.fix = ri() != 0;
    for (KeyFrame &k : c.kf)
        for (int r = 0; r < 3; ++r) for (int col = 0; col < 4; ++col) k.Tcw.at<float>(r, col) = (float)rd();
    for (KeyFrame &k : c.kf) read_K(k);
    std::vector<float> sig(8);
    for (float &v : sig) v = (float)rd();
    c.kf[0].mvLevelSigma2 = c.kf[1].mvLevelSigma2 = sig;
    std::vector<int> mp1((size_t)nk1);
    for (int i = 0; i < nk1; ++i) { cv::KeyPoint kp; kp.octave = ri(); mp1[i] = ri(); c.kf[0].mvKeysSemantic.push_back(kp); }
    for (int i = 0; i < nk2; ++i) { cv::KeyPoint kp; kp.octave = ri(); c.kf[1].mvKeysSemantic.push_back(kp); }
    c.pts.resize((size_t)np);
    for (MapPoint &p : c.pts) {
        for (int r = 0; r < 3; ++r) p.mWorldPos.at<float>(r, 0) = (float)rd();
        p.mbBad = ri() != 0; p.mnIndex[0] = ri(); p.mnIndex[1] = ri();
        p.mpKF[0] = &c.kf[0]; p.mpKF[1] = &c.kf[1];
    }
    for (int i = 0; i < nk1; ++i) c.kf[0].mvpMapPoints.push_back(mp1[i] >= 0 ? &c.pts[(size_t)mp1[i]] : nullptr);
    c.matches.resize((size_t)nm);
    for (int i = 0; i < nm; ++i) { const int m = ri(); c.matches[i] = m >= 0 ? &c.pts[(size_t)m] : nullptr; }
    c.solver.reset(new Sim3Solver(&c.kf[0], &c.kf[1], c.matches, c.fix));
}

static cv::Mat point(float x, float y, float z) {
    cv::Mat m(3, 1, CV_32F);
    m.at<float>(0) = x; m.at<float>(1) = y; m.at<float>(2) = z;
    return m;
}

// a solver whose correspondences are n given pairs: constructed over nothing, then the members of Sim3Solver.cc:86-110 filled in
static void fill_pairs(Sim3Solver &s, int n) {
    for (int i = 0; i < n; ++i) {
        float v[8];
        for (float &x : v) x = (float)rd();
        s.mvX3Dc1.push_back(point(v[0], v[1], v[2]));
        s.mvX3Dc2.push_back(point(v[3], v[4], v[5]));
        s.mvnMaxError1.push_back((size_t)v[6]);
        s.mvnMaxError2.push_back((size_t)v[7]);
        s.mvpMapPoints1.push_back(nullptr);
        s.mvpMapPoints2.push_back(nullptr);
        s.mvnIndices1.push_back((size_t)i);
        s.mvAllIndices.push_back((size_t)i);
    }
    s.mN1 = n;
    s.FromCameraToImage(s.mvX3Dc1, s.mvP1im1, s.mK1);
    s.FromCameraToImage(s.mvX3Dc2, s.mvP2im2, s.mK2);
}

static void print_rows(const cv::Mat &T) {
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) std::printf(" %a", T.at<float>(r, c));
}

static int core() {
    const int n = ri();
    const bool fix = ri() != 0;
    KeyFrame kf[2];
    read_K(kf[0]); read_K(kf[1]);
    std::vector<MapPoint *> none;
    Sim3Solver s(&kf[0], &kf[1], none, fix);
    fill_pairs(s, n);
    s.SetRansacParameters(0.99, 0, 1);            // N and mvbInliersi from the pairs
    const int nt = ri();
    cv::Mat P3Dc1i(3, 3, CV_32F), P3Dc2i(3, 3, CV_32F);
    for (int k = 0; k < nt; ++k) {
        for (int i = 0; i < 3; ++i) {
            const int idx = ri();
            s.mvX3Dc1[(size_t)idx].copyTo(P3Dc1i.col(i));
            s.mvX3Dc2[(size_t)idx].copyTo(P3Dc2i.col(i));
        }
        s.ComputeSim3(P3Dc1i, P3Dc2i);
        s.CheckInliers();
        std::vector<unsigned long long> words(((size_t)n + 63) / 64, 0);
        for (int i = 0; i < n; ++i)
            if (s.mvbInliersi[(size_t)i]) words[(size_t)i >> 6] |= 1ull << (i & 63);
        std::printf("%d", s.mnInliersi);
        for (int i = 0; i < 9; ++i) std::printf(" %a", s.mR12i.at<float>(i / 3, i % 3));
        for (int i = 0; i < 3; ++i) std::printf(" %a", s.mt12i.at<float>(i));
        std::printf(" %a", s.ms12i);
        print_rows(s.mT12i);
        print_rows(s.mT21i);
        for (unsigned long long x : words) std::printf(" %llx", x);
        std::printf("\n");
    }
    return 0;
}

static int params() {
    double N;
    while (std::scanf("%lf", &N) == 1) {
        KeyFrame kf[2];
        std::vector<MapPoint *> none;
        Sim3Solver s(&kf[0], &kf[1], none, true);
        s.mvpMapPoints1.assign((size_t)N, nullptr);
        const double prob = rd();
        const int minInliers = ri(), maxIts = ri();
        s.SetRansacParameters(prob, minInliers, maxIts);
        std::printf("%d\n", s.mRansacMaxIts);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "core") return core();
    if (mode == "params") return params();
    const int nc = ri();
    std::vector<std::unique_ptr<Candidate>> cands;
    for (int k = 0; k < nc; ++k) {
        cands.emplace_back(new Candidate);
        Candidate &c = *cands.back();
        read_candidate(c);
        if (mode == "run") {
            const double prob = rd();
            const int minInliers = ri(), maxIts = ri(), nd = ri();
            for (int i = 0; i < nd; ++i) c.script.draws.push_back(ri());
            c.solver->SetRansacParameters(prob, minInliers, maxIts);
        }
    }
    if (mode == "gather") {
        for (int k = 0; k < nc; ++k) {
            const Sim3Solver &s = *cands[k]->solver;
            for (size_t i = 0; i < s.mvnIndices1.size(); ++i) {
                std::printf("%d %zu", k, s.mvnIndices1[i]);
                for (int r = 0; r < 3; ++r) std::printf(" %a", s.mvX3Dc1[i].at<float>(r));
                for (int r = 0; r < 3; ++r) std::printf(" %a", s.mvX3Dc2[i].at<float>(r));
                std::printf(" %a %a", (float)s.mvnMaxError1[i], (float)s.mvnMaxError2[i]);
                std::printf(" %a %a %a %a\n", s.mvP1im1[i].at<float>(0), s.mvP1im1[i].at<float>(1), s.mvP2im2[i].at<float>(0), s.mvP2im2[i].at<float>(1));
            }
        }
        return 0;
    }
    if (mode == "run") {
        const int maxCalls = argc > 2 ? std::atoi(argv[2]) : 1000000;
        const int nIterations = argc > 3 ? std::atoi(argv[3]) : 5;
        bool shared = false, keep = false;
        for (int a = 4; a < argc; ++a) {
            shared = shared || std::string(argv[a]) == "shared";      // every candidate draws from the first one's list
            keep = keep || std::string(argv[a]) == "keep";            // a candidate that said bNoMore is called again
        }
        std::vector<int> calls((size_t)nc, 0);
        std::vector<bool> discarded((size_t)nc, false);
        int left = nc;
        while (left > 0) {
            for (int i = 0; i < nc; ++i) {
                if (discarded[i]) continue;
                std::vector<bool> vbInliers;
                int nInliers;
                bool bNoMore = false;
                Sim3Solver *pSolver = cands[i]->solver.get();
                DUtils::Random::current() = &cands[shared ? 0 : i]->script;
                cv::Mat Scm = nIterations > 0 ? pSolver->iterate(nIterations, bNoMore, vbInliers, nInliers) : pSolver->find(vbInliers, nInliers);
                if (nIterations == 0) bNoMore = true;         // (find() keeps its flag to itself; one call per candidate)
                if ((bNoMore && !keep) | (++calls[i] >= maxCalls)) { discarded[i] = true; left--; }
                std::printf("call %d %d %d %d %d\n", i, bNoMore ? 1 : 0, nInliers, Scm.empty() ? 0 : 1, pSolver->mRansacMaxIts);
                if (!Scm.empty()) {
                    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) std::printf("%a ", Scm.at<float>(r, c));
                    cv::Mat R = pSolver->GetEstimatedRotation(), t = pSolver->GetEstimatedTranslation();
                    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) std::printf("%a ", R.at<float>(r, c));
                    for (int r = 0; r < 3; ++r) std::printf("%a ", t.at<float>(r));
                    std::printf("%a\n", pSolver->GetEstimatedScale());
                    for (size_t j = 0; j < vbInliers.size(); ++j) std::printf("%d", vbInliers[j] ? 1 : 0);
                    std::printf("\n");
                }
            }
        }
        return 0;
    }
    return 2;
}
