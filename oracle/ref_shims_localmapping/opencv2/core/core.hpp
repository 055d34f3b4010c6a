// Stand-in for <opencv2/core/core.hpp> when the reference's LocalMapping.cc and MapPoint.cc are compiled for oracle/_ref: the cv::Mat
// of ref_shims_solvers (cv_min.hpp's CV_32F algebra with writable views) and what these two sources need beyond it, each stated from
// the rules cv_min.hpp gives for OpenCV 3.x:
//   * `s * A - B` and `A + B / s`: addWeighted with the weight narrowed to float (a * (float)s - b, a + b * (float)(1 / s));
//   * `-A * B.t() * c + d`, `A * B * C`: a product of two scaled operands is one gemm, a product whose left side is a product
//     evaluates that side first;
//   * cv::SVD::compute on the 4 x 4 float A and Mat::inv() of a 3 x 3 float matrix, which are the substitutions DESIGN.md §3.6e
//     states (oracle/cv_primitives.cpp; inv() is a member of the cv::Mat of ref_shims_solvers).  Of vt only row 3 is filled: the source reads nothing else (LocalMapping.cc:331).
// Test infrastructure only.
#pragma once
#include "../../../ref_shims_solvers/opencv2/core/core.hpp"

namespace cv {

// (a MatDiff, so that `A.row(i) = s * B.row(2) - B.row(0)` is written into A's storage: the product a * (float)s is one float rounding
// whether or not the difference follows in the same statement)
inline MatDiff operator-(const MatScaled &a, const Mat &b) { return MatDiff{MatCore(a), b}; }
inline Mat operator+(const Mat &a, const MatScaled &b) {
    Mat m(a.rows, a.cols, CV_32F);
    const float s = (float)b.alpha;
    for (int r = 0; r < a.rows; ++r)
        for (int c = 0; c < a.cols; ++c) m.at<float>(r, c) = a.at<float>(r, c) + (b.transposed ? b.m.at<float>(c, r) : b.m.at<float>(r, c)) * s;
    return m;
}
inline MatProduct operator*(const MatScaled &a, const MatScaled &b) { return MatProduct{a, b, MatCore(), 0.0}; }
inline MatProduct operator*(const MatProduct &p, const Mat &b) { return MatCore(p) * static_cast<const MatCore &>(b); }

class SVD {
 public:
    enum { MODIFY_A = 1, NO_UV = 2, FULL_UV = 4 };
    static void compute(const Mat &A, Mat &w, Mat &u, Mat &vt, int flags) {
        assert(A.rows == 4 && A.cols == 4 && A.type() == CV_32F && (flags & FULL_UV));
        float a[16], e[4];
        for (int i = 0; i < 16; ++i) a[i] = A.at<float>(i / 4, i % 4);
        cvp_null4(a, e);
        w = Mat::zeros(4, 1, CV_32F);
        u = Mat::zeros(4, 4, CV_32F);
        vt = Mat::zeros(4, 4, CV_32F);
        for (int i = 0; i < 4; ++i) vt.at<float>(3, i) = e[i];
    }
};

}  // namespace cv
