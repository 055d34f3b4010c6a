// Test program of tests/test_sim3_ransac_host.py and tests/test_gpu_sim3_ransac.py: SIVO::Sim3Solver over minimal KeyFrame / MapPoint
// stand-ins.  Reads loop candidates in text form on stdin (tests/sim3_ransac_restatement.py, scene_text), prints hex floats.
//   gather: the correspondences the constructor keeps (candidate, index in vpMatched12, x1c, x2c, max_err1, max_err2)
//   run:    per candidate `probability minInliers maxIterations ndraws draws...` follow the scene: one SolveAll, then the round-robin
//           iterate(5) of LoopClosing.cc:294-313 until every candidate has said bNoMore; every call is printed
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "orbslam/Sim3Solver.h"

struct TKeyFrame;
struct TMapPoint {
    cv::Mat pos = cv::Mat(3, 1, CV_32F);
    bool bad = false;
    int idx[2] = {-1, -1};             // GetIndexInKeyFrame(KF1), (KF2)
    TKeyFrame *kf[2] = {nullptr, nullptr};
    cv::Mat GetWorldPos() const { return pos; }
    bool isBad() const { return bad; }
    int GetIndexInKeyFrame(TKeyFrame *k) const { return k == kf[0] ? idx[0] : k == kf[1] ? idx[1] : -1; }
};
struct TKeyFrame {
    cv::Mat mK = cv::Mat::zeros(3, 3, CV_32F), Tcw = cv::Mat::zeros(4, 4, CV_32F);
    std::vector<cv::KeyPoint> mvKeysSemantic;
    std::vector<float> mvLevelSigma2;
    std::vector<TMapPoint *> mvpMapPoints;
    cv::Mat GetRotation() const { cv::Mat R(3, 3, CV_32F); for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R.at<float>(r, c) = Tcw.at<float>(r, c); return R; }
    cv::Mat GetTranslation() const { cv::Mat t(3, 1, CV_32F); for (int r = 0; r < 3; ++r) t.at<float>(r, 0) = Tcw.at<float>(r, 3); return t; }
    std::vector<TMapPoint *> GetMapPointMatches() const { return mvpMapPoints; }
};

static double rd() { double v; if (std::scanf("%lf", &v) != 1) std::exit(2); return v; }
static int ri() { return (int)rd(); }

struct Candidate {
    TKeyFrame kf[2];
    std::vector<TMapPoint> pts;
    std::vector<TMapPoint *> matches;
    bool fix = true;
    std::unique_ptr<SIVO::Sim3Solver> solver;
    std::vector<int> draws;
    size_t next = 0;
};

static void read_candidate(Candidate &c) {
    const int nk1 = ri(), nk2 = ri(), np = ri(), nm = ri();
    c.fix = ri() != 0;
    for (TKeyFrame &k : c.kf) {
        for (int r = 0; r < 3; ++r) for (int col = 0; col < 4; ++col) k.Tcw.at<float>(r, col) = (float)rd();
        k.Tcw.at<float>(3, 3) = 1.f;
    }
    for (TKeyFrame &k : c.kf) {
        k.mK.at<float>(0, 0) = (float)rd(); k.mK.at<float>(1, 1) = (float)rd(); k.mK.at<float>(0, 2) = (float)rd(); k.mK.at<float>(1, 2) = (float)rd();
        k.mK.at<float>(2, 2) = 1.f;
    }
    std::vector<float> sig(8);
    for (float &v : sig) v = (float)rd();
    c.kf[0].mvLevelSigma2 = c.kf[1].mvLevelSigma2 = sig;
    std::vector<int> mp1((size_t)nk1);
    for (int i = 0; i < nk1; ++i) { cv::KeyPoint kp; kp.octave = ri(); mp1[i] = ri(); c.kf[0].mvKeysSemantic.push_back(kp); }
    for (int i = 0; i < nk2; ++i) { cv::KeyPoint kp; kp.octave = ri(); c.kf[1].mvKeysSemantic.push_back(kp); }
    c.pts.resize((size_t)np);
    for (TMapPoint &p : c.pts) {
        for (int r = 0; r < 3; ++r) p.pos.at<float>(r, 0) = (float)rd();
        p.bad = ri() != 0; p.idx[0] = ri(); p.idx[1] = ri();
        p.kf[0] = &c.kf[0]; p.kf[1] = &c.kf[1];
    }
    for (int i = 0; i < nk1; ++i) c.kf[0].mvpMapPoints.push_back(mp1[i] >= 0 ? &c.pts[(size_t)mp1[i]] : nullptr);
    c.matches.resize((size_t)nm);
    for (int i = 0; i < nm; ++i) { const int m = ri(); c.matches[i] = m >= 0 ? &c.pts[(size_t)m] : nullptr; }
    c.solver.reset(new SIVO::Sim3Solver(&c.kf[0], &c.kf[1], c.matches, c.fix));
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    const int nc = ri();
    std::vector<std::unique_ptr<Candidate>> cands;
    for (int k = 0; k < nc; ++k) {
        cands.emplace_back(new Candidate);
        Candidate &c = *cands.back();
        read_candidate(c);
        if (mode == "run") {
            const double prob = rd();
            const int minInliers = ri(), maxIts = ri(), nd = ri();
            for (int i = 0; i < nd; ++i) c.draws.push_back(ri());
            c.solver->SetRansacParameters(prob, minInliers, maxIts);
            Candidate *pc = &c;
            c.solver->SetDraw([pc](int lo, int hi) {
                if (pc->next >= pc->draws.size()) std::exit(3);
                return lo + pc->draws[pc->next++] % (hi - lo + 1);
            });
        }
    }
    if (mode == "gather") {
        for (int k = 0; k < nc; ++k) {
            const SIVO::Sim3Solver &s = *cands[k]->solver;
            for (size_t i = 0; i < s.Pairs().size(); ++i) {
                const SivoSim3Pair &p = s.Pairs()[i];
                std::printf("%d %zu %a %a %a %a %a %a %a %a\n", k, s.Indices1()[i], p.x1c[0], p.x1c[1], p.x1c[2], p.x2c[0], p.x2c[1], p.x2c[2],
                            p.max_err1, p.max_err2);
            }
        }
        return 0;
    }
    if (mode == "run") {
        std::vector<SIVO::Sim3Solver *> solvers;
        for (auto &c : cands) solvers.push_back(c->solver.get());
        solvers.push_back(nullptr);                              // (a discarded candidate of LoopClosing.cc:270)
        SIVO::Sim3Solver::SolveAll(solvers);
        std::vector<bool> discarded((size_t)nc, false);
        int left = nc;
        while (left > 0) {
            for (int i = 0; i < nc; ++i) {
                if (discarded[i]) continue;
                std::vector<bool> vbInliers;
                int nInliers;
                bool bNoMore;
                SIVO::Sim3Solver *pSolver = solvers[i];
                cv::Mat Scm = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
                if (bNoMore) { discarded[i] = true; left--; }
                std::printf("call %d %d %d %d %d\n", i, bNoMore ? 1 : 0, nInliers, Scm.empty() ? 0 : 1, pSolver->MaxIterations());
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
