// SIVO::Sim3Solver — the reference class (reference include/orbslam/Sim3Solver.h:38-56, src/orbslam/Sim3Solver.cc) with its public
// interface, so that LoopClosing.cc:281-327 compiles against it unchanged: `new Sim3Solver(mpCurrentKF, pKF, vvpMapPointMatches[i],
// mbFixScale)`, `SetRansacParameters(0.99, 20, 300)`, `iterate(5, bNoMore, vbInliers, nInliers)`, `GetEstimated*()`.
//
// The constructor walks the SLAM objects exactly as Sim3Solver.cc:43-110 does and keeps arrays only.  Horn's closed form and the
// inlier test of EVERY hypothesis run on the device in one launch (sivo_sim3_ransac_batch, sivo_amd/csrc/sim3_ransac.hip): a
// solver draws all mRansacMaxIts samples at its first iterate / find, evaluates them at once, and iterate(n) replays the stored
// counts with the reference's sequential semantics — the returned cv::Mat, vbInliers, nInliers, bNoMore and GetEstimated*() are
// what the reference returns for the same samples.  Sim3Solver::SolveAll(vpSim3Solvers) in front of the round-robin loop of
// LoopClosing.cc:295 (the one optional line a caller adds) evaluates every candidate's solver in ONE launch.
//
// What differs from the reference: the ORDER in which the global random stream is consumed.  The reference draws three numbers
// per iteration as it goes, interleaving the candidates of the round-robin loop and stopping at the first acceptance; here a
// solver consumes 3 mRansacMaxIts draws at once when it is first evaluated.  For given samples the results are the same.
// Draws come from a settable functor int(int lo, int hi) (SetDraw); the default is a rand()-based uniform draw, a caller that
// links DBoW2 passes DUtils::Random::RandomInt.
// And one guard: a solver with fewer than 3 pairs says bNoMore at once (CanRun).  The reference asks only for N >= minInliers and
// with a smaller minInliers would draw from an empty mvAllIndices; LoopClosing.cc never builds such a solver (nmatches >= 20).
// (guard: NOT the reference's SIM3SOLVER_H — a translation unit may include the reference's header beside this one)
#ifndef SIVO_AMD_API_SIM3SOLVER_H
#define SIVO_AMD_API_SIM3SOLVER_H

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

class Sim3Solver {
 public:
    typedef std::function<int(int, int)> DrawFn;      // a uniform draw from [lo, hi], as DUtils::Random::RandomInt

    template <class KeyFrameT, class MapPointT>
    Sim3Solver(KeyFrameT *pKF1, KeyFrameT *pKF2, const std::vector<MapPointT *> &vpMatched12, const bool bFixScale = true);

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);

    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers);

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers);

    cv::Mat GetEstimatedRotation() { return mBestRotation.clone(); }
    cv::Mat GetEstimatedTranslation() { return mBestTranslation.clone(); }
    float GetEstimatedScale() { return mBestScale; }

    // ---- beyond the reference's interface
    void SetDraw(DrawFn draw) { mDraw = draw; }
    // Evaluates every solver of the list that is not yet evaluated (null entries skipped) in one launch.
    static void SolveAll(const std::vector<Sim3Solver *> &vpSolvers);
    // the gathered correspondences: pair k came from vpMatched12[Indices1()[k]]
    const std::vector<SivoSim3Pair> &Pairs() const { return mvPairs; }
    const std::vector<size_t> &Indices1() const { return mvnIndices1; }
    int MaxIterations() const { return mRansacMaxIts; }

 protected:
    static int DefaultDraw(int lo, int hi) {
        const int d = hi - lo + 1;
        return (int)(((double)std::rand() / ((double)RAND_MAX + 1.0)) * d) + lo;
    }
    // a double converted to int as the reference's build converts it (cvttsd2si): INT_MIN when not finite or out of range, where
    // the C++ conversion itself is undefined
    static int ToInt(double x) { return (std::isfinite(x) && x >= -2147483648.0 && x < 2147483648.0) ? (int)x : INT32_MIN; }
    bool CanRun() const { return N >= mRansacMinInliers && N >= 3; }      // (three pairs to sample from; the reference assumes them)
    void DrawSamples();

    std::vector<SivoSim3Pair> mvPairs;     // mvX3Dc1 / mvX3Dc2 / mvnMaxError1 / mvnMaxError2
    std::vector<size_t> mvnIndices1;
    float mK1[4], mK2[4];                  // fx fy cx cy
    int N = 0, mN1 = 0;
    bool mbFixScale;

    // the evaluated hypotheses
    bool mbEvaluated = false;
    std::vector<int32_t> mvTriples, mvCounts;
    std::vector<float> mvT;
    std::vector<uint64_t> mvBits;

    // Current Ransac State
    int mnIterations = 0, mnBestInliers = 0;
    cv::Mat mBestT12, mBestRotation, mBestTranslation;
    float mBestScale = 0.f;
    std::vector<bool> mvbBestInliers;

    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 300;
    DrawFn mDraw = &Sim3Solver::DefaultDraw;
};

template <class KeyFrameT, class MapPointT>
Sim3Solver::Sim3Solver(KeyFrameT *pKF1, KeyFrameT *pKF2, const std::vector<MapPointT *> &vpMatched12, const bool bFixScale)
    : mbFixScale(bFixScale) {
    const std::vector<MapPointT *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    mN1 = (int)vpMatched12.size();
    mvPairs.reserve(mN1);
    mvnIndices1.reserve(mN1);
    cv::Mat Rcw1 = pKF1->GetRotation();
    cv::Mat tcw1 = pKF1->GetTranslation();
    cv::Mat Rcw2 = pKF2->GetRotation();
    cv::Mat tcw2 = pKF2->GetTranslation();
    for (int i1 = 0; i1 < mN1; i1++) {
        if (vpMatched12[i1]) {
            MapPointT *pMP1 = vpKeyFrameMP1[i1];
            MapPointT *pMP2 = vpMatched12[i1];
            if (!pMP1) continue;
            if (pMP1->isBad() || pMP2->isBad()) continue;
            const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
            const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
            if (indexKF1 < 0 || indexKF2 < 0) continue;
            const cv::KeyPoint &kp1 = pKF1->mvKeysSemantic[indexKF1];
            const cv::KeyPoint &kp2 = pKF2->mvKeysSemantic[indexKF2];
            const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
            const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];
            SivoSim3Pair p;
            // the thresholds are unsigned long in the reference and convert to float in `err < mvnMaxError[i]`
            p.max_err1 = (float)static_cast<unsigned long>(9.210 * sigmaSquare1);
            p.max_err2 = (float)static_cast<unsigned long>(9.210 * sigmaSquare2);
            cv::Mat X3D1w = pMP1->GetWorldPos();
            cv::Mat X3D1c = Rcw1 * X3D1w + tcw1;
            cv::Mat X3D2w = pMP2->GetWorldPos();
            cv::Mat X3D2c = Rcw2 * X3D2w + tcw2;
            for (int r = 0; r < 3; ++r) { p.x1c[r] = X3D1c.at<float>(r); p.x2c[r] = X3D2c.at<float>(r); }
            mvPairs.push_back(p);
            mvnIndices1.push_back((size_t)i1);
        }
    }
    const cv::Mat K1 = pKF1->mK, K2 = pKF2->mK;
    mK1[0] = K1.at<float>(0, 0); mK1[1] = K1.at<float>(1, 1); mK1[2] = K1.at<float>(0, 2); mK1[3] = K1.at<float>(1, 2);
    mK2[0] = K2.at<float>(0, 0); mK2[1] = K2.at<float>(1, 1); mK2[2] = K2.at<float>(0, 2); mK2[3] = K2.at<float>(1, 2);
    SetRansacParameters();
}

inline void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    N = (int)mvPairs.size();      // number of correspondences
    // Adjust Parameters according to number of correspondences
    float epsilon = (float)mRansacMinInliers / N;
    // Set RANSAC iterations according to probability, epsilon, and max iterations
    int nIterations;
    if (mRansacMinInliers == N)
        nIterations = 1;
    else
        nIterations = ToInt(std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow((double)epsilon, 3.0))));
    mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
    mnIterations = 0;
    mbEvaluated = false;          // (the samples are drawn for mRansacMaxIts: drawn again at the next iterate)
}

// Sim3Solver.cc:166-180 for every iteration at once: three draws without replacement from mvAllIndices
inline void Sim3Solver::DrawSamples() {
    mvTriples.assign((size_t)3 * mRansacMaxIts, 0);
    std::vector<int32_t> vAvailableIndices;
    for (int h = 0; h < mRansacMaxIts; ++h) {
        vAvailableIndices.resize((size_t)N);
        for (int i = 0; i < N; ++i) vAvailableIndices[i] = i;
        for (short i = 0; i < 3; ++i) {
            const int randi = mDraw(0, (int)vAvailableIndices.size() - 1);
            mvTriples[(size_t)3 * h + i] = vAvailableIndices[randi];
            vAvailableIndices[randi] = vAvailableIndices.back();
            vAvailableIndices.pop_back();
        }
    }
}

inline void Sim3Solver::SolveAll(const std::vector<Sim3Solver *> &vpSolvers) {
    std::vector<Sim3Solver *> todo;
    std::vector<SivoSim3RansacProblem> probs;
    for (Sim3Solver *s : vpSolvers) {
        if (!s || s->mbEvaluated || !s->CanRun()) continue;
        bool listed = false;
        for (Sim3Solver *t : todo) listed = listed || t == s;
        if (listed) continue;
        s->DrawSamples();
        const size_t nh = (size_t)s->mRansacMaxIts, words = ((size_t)s->N + 63) / 64;
        s->mvCounts.assign(nh, 0); s->mvT.assign(13 * nh, 0.f); s->mvBits.assign(nh * words, 0);
        SivoSim3RansacProblem p = SivoSim3RansacProblem();
        p.pairs = s->mvPairs.data(); p.n = s->N;
        for (int i = 0; i < 4; ++i) { p.k1[i] = s->mK1[i]; p.k2[i] = s->mK2[i]; }
        p.triples = s->mvTriples.data(); p.n_hyp = s->mRansacMaxIts;
        p.min_inliers = s->mRansacMinInliers; p.fix_scale = s->mbFixScale ? 1 : 0;
        p.count = s->mvCounts.data(); p.T = s->mvT.data(); p.inlier_bits = s->mvBits.data();
        todo.push_back(s); probs.push_back(p);
    }
    if (todo.empty()) return;
    if (sivo_sim3_ransac_batch(probs.data(), (int)probs.size()) != SIVO_OK)
        throw std::runtime_error(std::string("Sim3Solver: ") + sivo_last_error());
    for (Sim3Solver *s : todo) s->mbEvaluated = true;
}

inline cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    if (!CanRun()) {
        bNoMore = true;
        return cv::Mat();
    }
    if (!mbEvaluated) SolveAll(std::vector<Sim3Solver *>(1, this));
    const size_t words = ((size_t)N + 63) / 64;
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
        nCurrentIterations++;
        mnIterations++;
        const size_t h = (size_t)mnIterations - 1;
        const int mnInliersi = mvCounts[h];
        if (mnInliersi >= mnBestInliers) {
            const float *T = &mvT[13 * h];
            const uint64_t *bits = words ? &mvBits[h * words] : nullptr;
            mvbBestInliers.assign((size_t)N, false);
            for (int i = 0; i < N; i++) mvbBestInliers[i] = (bits[i >> 6] >> (i & 63)) & 1;
            mnBestInliers = mnInliersi;
            mBestScale = T[12];
            mBestRotation = cv::Mat(3, 3, CV_32F);
            mBestTranslation = cv::Mat(3, 1, CV_32F);
            mBestT12 = cv::Mat::eye(4, 4, CV_32F);
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) {
                    mBestRotation.at<float>(r, c) = T[3 * r + c];
                    mBestT12.at<float>(r, c) = T[3 * r + c] * mBestScale;       // sR = ms12i * mR12i: a float product
                }
                mBestTranslation.at<float>(r, 0) = T[9 + r];
                mBestT12.at<float>(r, 3) = T[9 + r];
            }
            if (mnInliersi > mRansacMinInliers) {
                nInliers = mnInliersi;
                for (int i = 0; i < N; i++)
                    if (mvbBestInliers[i]) vbInliers[mvnIndices1[i]] = true;
                return mBestT12;
            }
        }
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;
    return cv::Mat();
}

inline cv::Mat Sim3Solver::find(std::vector<bool> &vbInliers12, int &nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

}  // namespace SIVO

#endif
