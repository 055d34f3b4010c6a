// Test program of tests/test_pnp_ransac_host.py and tests/test_gpu_pnp_ransac.py.  Reads text on stdin, prints hex floats.
//   core:   the kernel's arithmetic (sivo_amd/csrc/pnp_epnp.hpp) compiled for the host with a team of one: `n K[4]`, n points
//           (X Y Z u v max_err), `nsets`, then per set `m idx...`; per set EPnP on the set and CheckInliers over all points are
//           printed (count, [R | t] as floats, the inlier words)
//   core64: the same with [R | t] as the doubles the arithmetic holds (tests/test_pin_solvers.py)
//   gather / run: SIVO::PnPsolver over minimal Frame / MapPoint stand-ins; candidates in the text form of
//           tests/pnp_ransac_restatement.py frame_text
//   gather: the correspondences the constructor keeps after SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) (candidate, index in
//           vpMapPointMatches, xw, u, v, max_err)
//   run:    per candidate `probability minInliers maxIterations epsilon th2 ndraws draws...` follow the frame: one SolveAll, then the
//           round-robin iterate(5) of Tracking.cc:1293-1310 until every candidate has said bNoMore (or was called argv[2] times);
//           every call is printed
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "orbslam/PnPsolver.h"
#include "pnp_epnp.hpp"

struct TMapPoint {
    cv::Mat pos = cv::Mat(3, 1, CV_32F);
    bool bad = false;
    cv::Mat GetWorldPos() const { return pos; }
    bool isBad() const { return bad; }
};
struct TFrame {
    float fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<cv::KeyPoint> mvKeysSemantic;
    std::vector<float> mvLevelSigma2;
    std::vector<TMapPoint *> mvpMapPoints;
};

static double rd() { double v; if (std::scanf("%lf", &v) != 1) std::exit(2); return v; }
static int ri() { return (int)rd(); }

struct Candidate {
    TFrame F;
    std::vector<TMapPoint> pts;
    std::vector<TMapPoint *> matches;
    std::unique_ptr<SIVO::PnPsolver> solver;
    std::vector<int> draws;
    size_t next = 0;
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
    for (TMapPoint &p : c.pts) {
        for (int r = 0; r < 3; ++r) p.pos.at<float>(r, 0) = (float)rd();
        p.bad = ri() != 0;
    }
    for (int i = 0; i < nk; ++i) c.matches.push_back(m[i] >= 0 ? &c.pts[(size_t)m[i]] : nullptr);
    c.F.mvpMapPoints.assign((size_t)nk, nullptr);
    c.solver.reset(new SIVO::PnPsolver(c.F, c.matches));
}

static int core(bool doubles) {
    const int n = ri();
    const double K[4] = {(double)(float)rd(), (double)(float)rd(), (double)(float)rd(), (double)(float)rd()};
    std::vector<SivoPnpPoint> pts((size_t)n);
    for (SivoPnpPoint &p : pts) {
        p.xw[0] = (float)rd(); p.xw[1] = (float)rd(); p.xw[2] = (float)rd();
        p.u = (float)rd(); p.v = (float)rd(); p.max_err = (float)rd();
    }
    const int nsets = ri();
    std::unique_ptr<sivo::PnpWork> w(new sivo::PnpWork);
    for (int s = 0; s < nsets; ++s) {
        const int m = ri();
        std::vector<int32_t> idx((size_t)m);
        for (int32_t &i : idx) i = ri();
        const int sol = sivo::pnp_epnp(sivo::PnpHostTeam(), *w, pts.data(), idx.data(), m, K);
        int count = 0;
        std::vector<unsigned long long> words(((size_t)n + 63) / 64, 0);
        for (int i = 0; i < n; ++i) {
            const SivoPnpPoint &p = pts[(size_t)i];
            if (sivo::pnp_inlier(w->Rs[sol], w->ts[sol], K, p.xw[0], p.xw[1], p.xw[2], p.u, p.v, p.max_err)) {
                ++count;
                words[(size_t)i >> 6] |= 1ull << (i & 63);
            }
        }
        std::printf("%d", count);
        for (int i = 0; i < 12; ++i) {
            const double v = i < 9 ? w->Rs[sol][i] : w->ts[sol][i - 9];
            std::printf(" %a", doubles ? v : (double)(float)v);
        }
        for (unsigned long long x : words) std::printf(" %llx", x);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "core" || mode == "core64") return core(mode == "core64");
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
            for (int i = 0; i < nd; ++i) c.draws.push_back(ri());
            c.solver->SetRansacParameters(prob, minInliers, maxIts, 4, eps, th2);
            Candidate *pc = &c;
            c.solver->SetDraw([pc](int lo, int hi) {
                if (pc->next >= pc->draws.size()) std::exit(3);
                return lo + pc->draws[pc->next++] % (hi - lo + 1);
            });
        } else {
            c.solver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
        }
    }
    if (mode == "gather") {
        for (int k = 0; k < nc; ++k) {
            const SIVO::PnPsolver &s = *cands[k]->solver;
            for (size_t i = 0; i < s.Points().size(); ++i) {
                const SivoPnpPoint &p = s.Points()[i];
                std::printf("%d %zu %a %a %a %a %a %a\n", k, s.KeyPointIndices()[i], p.xw[0], p.xw[1], p.xw[2], p.u, p.v, p.max_err);
            }
        }
        return 0;
    }
    if (mode == "run") {
        std::vector<SIVO::PnPsolver *> vpPnPsolvers;
        for (auto &c : cands) vpPnPsolvers.push_back(c->solver.get());
        vpPnPsolvers.push_back(nullptr);                         // (a discarded candidate of Tracking.cc:1270)
        SIVO::PnPsolver::SolveAll(vpPnPsolvers);
        std::vector<bool> vbDiscarded((size_t)nc, false);
        std::vector<int> calls((size_t)nc, 0);
        const int maxCalls = argc > 2 ? std::atoi(argv[2]) : 1000;   // (a candidate that keeps accepting never says bNoMore)
        int nCandidates = nc;
        while (nCandidates > 0) {
            for (int i = 0; i < nc; ++i) {
                if (vbDiscarded[i]) continue;
                std::vector<bool> vbInliers;
                int nInliers;
                bool bNoMore;
                SIVO::PnPsolver *pSolver = vpPnPsolvers[i];
                cv::Mat Tcw = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
                if (bNoMore || ++calls[i] >= maxCalls) { vbDiscarded[i] = true; nCandidates--; }
                std::printf("call %d %d %d %d %d %d\n", i, bNoMore ? 1 : 0, nInliers, Tcw.empty() ? 0 : 1, pSolver->MaxIterations(),
                            pSolver->MinInliers());
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
