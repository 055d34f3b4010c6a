// SIVO::PnPsolver — the reference class (reference include/orbslam/PnPsolver.h:65-89, src/orbslam/PnPsolver.cc) with its public
// interface, so that Tracking.cc:1279-1304 compiles against it unchanged: `new PnPsolver(mCurrentFrame, vvpMapPointMatches[i])`,
// `SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)`, `iterate(5, bNoMore, vbInliers, nInliers)`.
//
// The constructor walks the SLAM objects exactly as PnPsolver.cc:72-121 does and keeps arrays only.  EPnP and the inlier test of
// EVERY hypothesis, and Refine of every running best, run on the device (sivo_pnp_ransac_batch, sivo_amd/csrc/pnp_ransac.hip): a
// solver draws all mRansacMaxIts samples when it is first evaluated, and iterate(n) replays the stored results with the reference's
// sequential semantics — the returned cv::Mat, vbInliers, nInliers and bNoMore are what the reference returns for the same samples.
// PnPsolver::SolveAll(vpPnPsolvers) in front of the loop of Tracking.cc:1293 (the one optional line a caller adds) evaluates every
// candidate's solver in ONE call.  The reference's loop condition is an OR (:198): a call made after mRansacMaxIts iterations runs
// nIterations further ones; the solver then draws and evaluates exactly that many more, in one further call.
//
// What differs from the reference:
//   * the ORDER in which the global random stream is consumed.  The reference draws four numbers per iteration as it goes,
//     interleaving the candidates of the round-robin loop and stopping at an acceptance; here a solver consumes 4 mRansacMaxIts
//     draws at once when it is first evaluated.  For given samples the results are the same.  Draws come from a settable functor
//     int(int lo, int hi) (SetDraw); the default is a rand()-based uniform draw, a caller that links DBoW2 passes
//     DUtils::Random::RandomInt;
//   * minSet != 4 throws std::invalid_argument (the device's hypothesis kernel is EPnP on four correspondences; the only caller,
//     Tracking.cc:1281, passes 4);
//   * a solver with fewer than 4 correspondences says bNoMore at once (the reference would draw from an empty vector).
// (guard: NOT the reference's PNPSOLVER_H — a translation unit may include the reference's header beside this one)
#ifndef SIVO_AMD_API_PNPSOLVER_H
#define SIVO_AMD_API_PNPSOLVER_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/sivo_hip.h"

#ifdef SIVO_HAVE_OPENCV
#include <opencv2/core/core.hpp>
#else
#include "../compat/cv_min.hpp"
#endif

namespace SIVO {

class PnPsolver {
 public:
    typedef std::function<int(int, int)> DrawFn;      // a uniform draw from [lo, hi], as DUtils::Random::RandomInt

    template <class FrameT, class MapPointT>
    PnPsolver(const FrameT &F, const std::vector<MapPointT *> &vpMapPointMatches);

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                             float epsilon = 0.4, float th2 = 5.991);

    cv::Mat find(std::vector<bool> &vbInliers, int &nInliers);

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    // ---- beyond the reference's interface
    void SetDraw(DrawFn draw) { mDraw = draw; }
    // Evaluates every solver of the list that is not yet evaluated (null entries skipped) in one call.
    static void SolveAll(const std::vector<PnPsolver *> &vpSolvers);
    // the gathered correspondences: point k came from vpMapPointMatches[KeyPointIndices()[k]]
    const std::vector<SivoPnpPoint> &Points() const { return mvPoints; }
    const std::vector<size_t> &KeyPointIndices() const { return mvKeyPointIndices; }
    int MaxIterations() const { return mRansacMaxIts; }
    int MinInliers() const { return mRansacMinInliers; }

 protected:
    static int DefaultDraw(int lo, int hi) {
        const int d = hi - lo + 1;
        return (int)(((double)std::rand() / ((double)RAND_MAX + 1.0)) * d) + lo;
    }
    // a double converted to int as the reference's build converts it (cvttsd2si): INT_MIN when not finite or out of range, where
    // the C++ conversion itself is undefined
    static int ToInt(double x) { return (std::isfinite(x) && x >= -2147483648.0 && x < 2147483648.0) ? (int)x : INT32_MIN; }
    bool CanRun() const { return N >= mRansacMinInliers && N >= 4; }
    // draws nHyp more samples (:203-220) and fills a problem that evaluates them behind the ones already held
    SivoPnpRansacProblem Extend(int nHyp);
    static void Evaluate(std::vector<SivoPnpRansacProblem> &probs);
    static cv::Mat ToMat(const float *T);

    std::vector<SivoPnpPoint> mvPoints;    // mvP3Dw / mvP2D / mvMaxError
    std::vector<float> mvSigma2;
    std::vector<size_t> mvKeyPointIndices;
    size_t mnMatches = 0;                  // mvpMapPointMatches.size()
    float mK[4];                           // fx fy cx cy
    int N = 0;

    // the evaluated hypotheses, in the order drawn
    std::vector<int32_t> mvSamples, mvCounts, mvRefined;
    std::vector<float> mvT, mvRefinedT;
    std::vector<uint64_t> mvBits, mvRefinedBits;

    // Current Ransac State
    int mnIterations = 0, mnBestInliers = 0;
    cv::Mat mBestTcw;
    std::vector<bool> mvbBestInliers;
    // Refine of the running best (a pure function of mvbBestInliers): the record's refinement
    int mnRefinedInliers = 0;
    cv::Mat mRefinedTcw;
    std::vector<bool> mvbRefinedInliers;

    double mRansacProb = 0.99;
    int mRansacMinInliers = 8, mRansacMaxIts = 300, mRansacMinSet = 4;
    float mRansacEpsilon = 0.4f;
    DrawFn mDraw = &PnPsolver::DefaultDraw;
};

template <class FrameT, class MapPointT>
PnPsolver::PnPsolver(const FrameT &F, const std::vector<MapPointT *> &vpMapPointMatches) {
    mnMatches = vpMapPointMatches.size();
    mvPoints.reserve(F.mvpMapPoints.size());
    mvSigma2.reserve(F.mvpMapPoints.size());
    mvKeyPointIndices.reserve(F.mvpMapPoints.size());
    for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
        MapPointT *pMP = vpMapPointMatches[i];
        if (pMP) {
            if (!pMP->isBad()) {
                const cv::KeyPoint &kp = F.mvKeysSemantic[i];
                SivoPnpPoint p;
                p.u = kp.pt.x; p.v = kp.pt.y;
                p.max_err = 0.f;
                mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
                cv::Mat Pos = pMP->GetWorldPos();
                p.xw[0] = Pos.at<float>(0); p.xw[1] = Pos.at<float>(1); p.xw[2] = Pos.at<float>(2);
                mvPoints.push_back(p);
                mvKeyPointIndices.push_back(i);
            }
        }
    }
    // Set camera calibration parameters
    mK[0] = F.fx; mK[1] = F.fy; mK[2] = F.cx; mK[3] = F.cy;
    SetRansacParameters();
}

inline void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, float th2) {
    if (minSet != 4) throw std::invalid_argument("PnPsolver: the device evaluates samples of 4 correspondences (minSet == 4)");
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    mRansacEpsilon = epsilon;
    mRansacMinSet = minSet;
    N = (int)mvPoints.size();     // number of correspondences
    // Adjust Parameters according to number of correspondences
    int nMinInliers = ToInt(N * mRansacEpsilon);
    if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    mRansacMinInliers = nMinInliers;
    if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
    // Set RANSAC iterations according to probability, epsilon, and max iterations
    int nIterations;
    if (mRansacMinInliers == N)
        nIterations = 1;
    else
        nIterations = ToInt(std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow((double)mRansacEpsilon, 3.0))));
    mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
    for (size_t i = 0; i < mvSigma2.size(); i++) mvPoints[i].max_err = mvSigma2[i] * th2;
    // (the samples held were evaluated against the former thresholds: a solver not yet iterated starts over)
    if (mnIterations == 0) { mvSamples.clear(); mvCounts.clear(); mvRefined.clear(); mvT.clear(); mvRefinedT.clear(); mvBits.clear(); mvRefinedBits.clear(); }
}

inline SivoPnpRansacProblem PnPsolver::Extend(int nHyp) {
    const size_t have = mvCounts.size(), nh = have + (size_t)nHyp, words = ((size_t)N + 63) / 64;
    mvSamples.resize(4 * nh);
    std::vector<int32_t> vAvailableIndices;
    for (size_t h = have; h < nh; ++h) {
        vAvailableIndices.resize((size_t)N);
        for (int i = 0; i < N; ++i) vAvailableIndices[i] = i;
        for (short i = 0; i < 4; ++i) {
            const int randi = mDraw(0, (int)vAvailableIndices.size() - 1);
            mvSamples[4 * h + i] = vAvailableIndices[randi];
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }
    mvCounts.resize(nh, 0); mvRefined.resize(nh, -1); mvT.resize(12 * nh, 0.f); mvRefinedT.resize(12 * nh, 0.f);
    mvBits.resize(nh * words, 0); mvRefinedBits.resize(nh * words, 0);
    SivoPnpRansacProblem p = SivoPnpRansacProblem();
    p.points = mvPoints.data(); p.n = N;
    for (int i = 0; i < 4; ++i) p.K[i] = mK[i];
    p.min_inliers = mRansacMinInliers;
    p.samples = mvSamples.data() + 4 * have; p.n_hyp = nHyp;
    p.count = mvCounts.data() + have; p.T = mvT.data() + 12 * have; p.inlier_bits = mvBits.data() + have * words;
    p.refined = mvRefined.data() + have; p.refined_T = mvRefinedT.data() + 12 * have; p.refined_bits = mvRefinedBits.data() + have * words;
    return p;
}

inline void PnPsolver::Evaluate(std::vector<SivoPnpRansacProblem> &probs) {
    if (sivo_pnp_ransac_batch(probs.data(), (int)probs.size()) != SIVO_OK)
        throw std::runtime_error(std::string("PnPsolver: ") + sivo_last_error());
}

inline void PnPsolver::SolveAll(const std::vector<PnPsolver *> &vpSolvers) {
    std::vector<PnPsolver *> todo;
    std::vector<SivoPnpRansacProblem> probs;
    for (PnPsolver *s : vpSolvers) {
        if (!s || !s->mvCounts.empty() || !s->CanRun()) continue;
        if (std::find(todo.begin(), todo.end(), s) != todo.end()) continue;
        SivoPnpRansacProblem p = s->Extend(s->mRansacMaxIts);
        p.best_in = 0;
        todo.push_back(s); probs.push_back(p);
    }
    if (!todo.empty()) Evaluate(probs);
}

inline cv::Mat PnPsolver::ToMat(const float *T) {
    cv::Mat M = cv::Mat::eye(4, 4, CV_32F);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) M.at<float>(r, c) = T[3 * r + c];
        M.at<float>(r, 3) = T[9 + r];
    }
    return M;
}

inline cv::Mat PnPsolver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    if (!CanRun()) {
        bNoMore = true;
        return cv::Mat();
    }
    if (mvCounts.empty()) SolveAll(std::vector<PnPsolver *>(1, this));
    const size_t words = ((size_t)N + 63) / 64;
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {
        if ((size_t)mnIterations == mvCounts.size()) {
            // past the samples held (the OR above: mnIterations >= mRansacMaxIts here): what is left of this call, in one call
            std::vector<SivoPnpRansacProblem> probs(1, Extend(nIterations - nCurrentIterations));
            probs[0].best_in = mnBestInliers;
            Evaluate(probs);
        }
        nCurrentIterations++;
        mnIterations++;
        const size_t h = (size_t)mnIterations - 1;
        const int mnInliersi = mvCounts[h];
        if (mnInliersi >= mRansacMinInliers) {
            // If it is the best solution so far, save it (a record: the device refined it)
            if (mnInliersi > mnBestInliers) {
                const uint64_t *bits = &mvBits[h * words], *rbits = &mvRefinedBits[h * words];
                mvbBestInliers.assign((size_t)N, false);
                mvbRefinedInliers.assign((size_t)N, false);
                for (int i = 0; i < N; i++) {
                    mvbBestInliers[i] = (bits[i >> 6] >> (i & 63)) & 1;
                    mvbRefinedInliers[i] = (rbits[i >> 6] >> (i & 63)) & 1;
                }
                mnBestInliers = mnInliersi;
                mBestTcw = ToMat(&mvT[12 * h]);
                mnRefinedInliers = mvRefined[h];
                mRefinedTcw = ToMat(&mvRefinedT[12 * h]);
            }
            // Refine() (:271-315)
            if (mnRefinedInliers > mRansacMinInliers) {
                nInliers = mnRefinedInliers;
                vbInliers = std::vector<bool>(mnMatches, false);
                for (int i = 0; i < N; i++)
                    if (mvbRefinedInliers[i]) vbInliers[mvKeyPointIndices[i]] = true;
                return mRefinedTcw.clone();
            }
        }
    }
    if (mnIterations >= mRansacMaxIts) {
        bNoMore = true;
        if (mnBestInliers >= mRansacMinInliers) {
            nInliers = mnBestInliers;
            vbInliers = std::vector<bool>(mnMatches, false);
            for (int i = 0; i < N; i++)
                if (mvbBestInliers[i]) vbInliers[mvKeyPointIndices[i]] = true;
            return mBestTcw.clone();
        }
    }
    return cv::Mat();
}

inline cv::Mat PnPsolver::find(std::vector<bool> &vbInliers, int &nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
}

}  // namespace SIVO

#endif
