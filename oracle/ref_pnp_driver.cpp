// Driver of the reference's OWN PnPsolver (src/orbslam/PnPsolver.cc, compiled untouched into oracle/_ref/ref_pnpsolver.o with its
// private members made reachable) for tests/test_pin_solvers.py.  It speaks the text protocols of tests/pnp_ransac_prog.cpp: text on
// stdin, hex floats out.
//   core:   `n K[4]`, n points (X Y Z u v max_err), `nsets`, per set `m idx...`.  Per set the reference's reset_correspondences /
//           add_correspondence / compute_pose / CheckInliers; printed: count, R (9) and t (3) as the doubles mRi / mti hold, the
//           inlier words
//   gather: candidates in the frame text form; after SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) what the constructor kept:
//           candidate, mvKeyPointIndices, mvP3Dw, mvP2D, mvMaxError, mvSigma2
//   run:    per candidate `probability minInliers maxIterations epsilon th2 ndraws draws...` follow the frame; the round-robin of
//           Tracking.cc:1293-1310 until every candidate said bNoMore or was called argv[2] times, iterate(argv[3], default 5) per
//           call (0: find()); every call is printed as pnp_ransac_prog prints it.  DUtils::Random::RandomInt reads the draws of
//           the candidate being called.  Further arguments: "shared" (every candidate draws from the first one's list: one stream for
//           all, as the reference's global one), "keep" (a candidate is called again after bNoMore, until argv[2] calls)
//   params: lines `N probability minInliers maxIterations minSet epsilon`: mRansacMinInliers, mRansacMaxIts and mRansacEpsilon
//           after SetRansacParameters on a solver of N correspondences
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "include/orbslam/PnPsolver.h"
#include "dependencies/DBoW2/DUtils/Random.h"

using SIVO::Frame;
using SIVO::MapPoint;
using SIVO::PnPsolver;

static double rd() { double v; if (std::scanf("%lf", &v) != 1) std::exit(2); return v; }
static int ri() { return (int)rd(); }

struct Candidate {
    Frame F;
    std::vector<MapPoint> pts;
    std::vector<MapPoint *> matches;
    std::unique_ptr<PnPsolver> solver;
    DUtils::Random::Script script;
};

static void read_candidate(Candidate &c) {
    c.F.fx = (float)rd(); c.F.fy = (float)rd(); c.F.cx = (float)rd(); c.F.cy = (float)rd();
    const int nk = ri(), np = ri();
    c.F.mvLevelSigma2.resize(8);
    for (float &v : c.F.mvLevelSigma2) v = (float)rd();
    std::vector<int> m((size_t)nk);
    for (int i = 0; i < nk; ++i) {
        cv::KeyPoint kp;
        kp.pt.x = (float)rd(); kp.pt.y = (float)rd(); kp.octave = ri(); m[i] = ri();
        c.F.mvKeysSemantic.push_back(kp);
    }
    c.pts.resize((size_t)np);
    for (MapPoint &p : c.pts) {
        for (int r = 0; r < 3; ++r) p.mWorldPos.at<float>(r, 0) = (float)rd();
        p.mbBad = ri() != 0;
    }
    for (int i = 0; i < nk; ++i) c.matches.push_back(m[i] >= 0 ? &c.pts[(size_t)m[i]] : nullptr);
    c.F.mvpMapPoints.assign((size_t)nk, nullptr);
    c.solver.reset(new PnPsolver(c.F, c.matches));
}

// a solver over n given correspondences: a frame whose every key has a good map point
static void plain_candidate(Candidate &c, int n) {
    c.F.mvLevelSigma2.assign(8, 1.0f);
    c.pts.resize((size_t)n);
    c.F.mvKeysSemantic.resize((size_t)n);
    for (int i = 0; i < n; ++i) c.matches.push_back(&c.pts[(size_t)i]);
    c.F.mvpMapPoints.assign((size_t)n, nullptr);
}

static int core() {
    const int n = ri();
    Candidate c;
    c.F.fx = (float)rd(); c.F.fy = (float)rd(); c.F.cx = (float)rd(); c.F.cy = (float)rd();
    plain_candidate(c, n);
    std::vector<float> max_err((size_t)n);
    for (int i = 0; i < n; ++i) {
        for (int r = 0; r < 3; ++r) c.pts[(size_t)i].mWorldPos.at<float>(r, 0) = (float)rd();
        c.F.mvKeysSemantic[(size_t)i].pt.x = (float)rd(); c.F.mvKeysSemantic[(size_t)i].pt.y = (float)rd();
        max_err[(size_t)i] = (float)rd();
    }
    PnPsolver s(c.F, c.matches);
    if (s.N != n) return 4;
    s.mvMaxError = max_err;                       // the thresholds as given (SetRansacParameters would derive them from the octave)
    const int nsets = ri();
    for (int k = 0; k < nsets; ++k) {
        const int m = ri();
        s.set_maximum_number_of_correspondences(m);
        s.reset_correspondences();
        for (int j = 0; j < m; ++j) {
            const int idx = ri();
            s.add_correspondence(s.mvP3Dw[idx].x, s.mvP3Dw[idx].y, s.mvP3Dw[idx].z, s.mvP2D[idx].x, s.mvP2D[idx].y);
        }
        s.compute_pose(s.mRi, s.mti);
        s.CheckInliers();
        std::vector<unsigned long long> words(((size_t)n + 63) / 64, 0);
        for (int i = 0; i < n; ++i)
            if (s.mvbInliersi[(size_t)i]) words[(size_t)i >> 6] |= 1ull << (i & 63);
        std::printf("%d", s.mnInliersi);
        for (int i = 0; i < 9; ++i) std::printf(" %a", s.mRi[i / 3][i % 3]);
        for (int i = 0; i < 3; ++i) std::printf(" %a", s.mti[i]);
        for (unsigned long long x : words) std::printf(" %llx", x);
        std::printf("\n");
    }
    return 0;
}

static int params() {
    double N;
    while (std::scanf("%lf", &N) == 1) {
        Candidate c;
        plain_candidate(c, (int)N);
        PnPsolver s(c.F, c.matches);
        const double prob = rd();
        const int minInliers = ri(), maxIts = ri(), minSet = ri();
        const float eps = (float)rd();
        s.SetRansacParameters(prob, minInliers, maxIts, minSet, eps, 5.991f);
        std::printf("%d %d %a\n", s.mRansacMinInliers, s.mRansacMaxIts, s.mRansacEpsilon);
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
            const int minInliers = ri(), maxIts = ri();
            const float eps = (float)rd(), th2 = (float)rd();
            const int nd = ri();
            for (int i = 0; i < nd; ++i) c.script.draws.push_back(ri());
            c.solver->SetRansacParameters(prob, minInliers, maxIts, 4, eps, th2);
        } else {
            c.solver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        }
    }
    if (mode == "gather") {
        for (int k = 0; k < nc; ++k) {
            const PnPsolver &s = *cands[k]->solver;
            for (size_t i = 0; i < s.mvP2D.size(); ++i)
                std::printf("%d %zu %a %a %a %a %a %a %a\n", k, s.mvKeyPointIndices[i], s.mvP3Dw[i].x, s.mvP3Dw[i].y, s.mvP3Dw[i].z, s.mvP2D[i].x,
                            s.mvP2D[i].y, s.mvMaxError[i], s.mvSigma2[i]);
        }
        return 0;
    }
    if (mode == "run") {
        std::vector<bool> vbDiscarded((size_t)nc, false);
        std::vector<int> calls((size_t)nc, 0);
        const int maxCalls = argc > 2 ? std::atoi(argv[2]) : 1000;
        const int nIterations = argc > 3 ? std::atoi(argv[3]) : 5;
        bool shared = false, keep = false;
        for (int a = 4; a < argc; ++a) {
            shared = shared || std::string(argv[a]) == "shared";      // every candidate draws from the first one's list
            keep = keep || std::string(argv[a]) == "keep";            // a candidate that said bNoMore is called again
        }
        int nCandidates = nc;
        while (nCandidates > 0) {
            for (int i = 0; i < nc; ++i) {
                if (vbDiscarded[i]) continue;
                std::vector<bool> vbInliers;
                int nInliers;
                bool bNoMore = false;
                PnPsolver *pSolver = cands[i]->solver.get();
                DUtils::Random::current() = &cands[shared ? 0 : i]->script;
                cv::Mat Tcw = nIterations > 0 ? pSolver->iterate(nIterations, bNoMore, vbInliers, nInliers) : pSolver->find(vbInliers, nInliers);
                if (nIterations == 0) bNoMore = true;         // (find() keeps its flag to itself; one call per candidate)
                if ((bNoMore && !keep) | (++calls[i] >= maxCalls)) { vbDiscarded[i] = true; nCandidates--; }
                std::printf("call %d %d %d %d %d %d\n", i, bNoMore ? 1 : 0, nInliers, Tcw.empty() ? 0 : 1, pSolver->mRansacMaxIts,
                            pSolver->mRansacMinInliers);
                if (!Tcw.empty()) {
                    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) std::printf("%a ", Tcw.at<float>(r, c));
                    std::printf("\n");
                    for (size_t j = 0; j < vbInliers.size(); ++j) std::printf("%d", vbInliers[j] ? 1 : 0);
                    std::printf("\n");
                }
            }
        }
        return 0;
    }
    return 2;
}
