/* The OpenCV primitives under the reference's PnPsolver.cc, Sim3Solver.cc and LocalMapping.cc, as the substitutions DESIGN.md §3.6c /
 * §3.6d / §3.6e state, written once in plain C++ (cv_primitives.cpp) for the reference build of oracle/_ref and for tests/test_pin_solvers.py.
 * A third statement of them, independent of the kernels' headers and of the numpy restatements.  All matrices row-major. */
#pragma once
#ifdef __cplusplus
extern "C" {
#endif
/* cvMulTransposed(src, dst, 1): dst (cols x cols) = src' src, every entry the sum over the rows in order */
void cvp_mul_transposed(const double *src, int rows, int cols, double *dst);
/* cyclic Jacobi on the symmetric A (m x m, overwritten), V (m x m) starting from the identity: `sweeps` sweeps over the pairs
 * (0,1) (0,2) .. (m-2,m-1), a rotation skipped when its off-diagonal entry is exactly zero; column k of V is the k-th eigenvector */
void cvp_jacobi(double *A, double *V, int m, int sweeps);
/* order[k] = index of the k-th largest |d|; ties, and everything that does not compare, to the lower index */
void cvp_order(const double *d, int m, int *order);
/* cvSVD(A, W, Ut, 0, CV_SVD_MODIFY_A | CV_SVD_U_T) of a symmetric A (m = 3 or 12): W the diagonal after the Jacobi in that order,
 * row k of Ut the eigenvector that belongs to W[k] */
void cvp_svd_symmetric(double *A, int m, double *W, double *Ut);
/* cvSVD(A, W, U, V, CV_SVD_MODIFY_A) of a general 3 x 3: one-sided Jacobi over the column pairs (0,1) (0,2) (1,2); W the column
 * norms (unordered), U the rotated columns over them (0 / 0 where a norm is zero), V the accumulated rotations: A = U diag(W) V' */
void cvp_svd3(double *A, double *W, double *U, double *V);
/* cvSolve(A, b, x, CV_SVD) on an nr x nc system (nc <= nr <= 8): the reference's Householder qr_solve scheme on copies (its scan for the
 * column maximum included, which sees rows k .. nr-2); x is NaN where that scheme returns early on a zero column */
void cvp_solve(const double *A, int nr, int nc, const double *b, double *x);
/* cvInvert(A, Ainv, CV_SVD) of a 3 x 3: adjugate over determinant */
void cvp_invert3(const double *A, double *Ainv);
/* cv::eigen of the symmetric 4 x 4 float N: Jacobi in double, eigenpairs by descending eigenvalue (ties to the lower index),
 * rounded to float; row k of evec is the k-th eigenvector */
void cvp_eigen4(const float *N, float *eval, float *evec);
/* atan2 + cv::Rodrigues of Sim3Solver.cc:293-300 as the rotation matrix of the quaternion q = (w, x, y, z), normalised, formed in
 * double and rounded once; NaN where the imaginary part is zero (the reference's axis is 0 / 0 there) */
void cvp_quaternion_rotation(const float *q, float *R);
/* the sweep counts compiled in: 3 x 3, 12 x 12, one-sided, 4 x 4 */
void cvp_sweeps(int *out4);
/* cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) of the 4 x 4 float A of LocalMapping.cc:321-331, of which the source uses vt.row(3)
 * alone, as the substitution DESIGN.md §3.6e states: e = the eigenvector of the smallest eigenvalue (ties to the lower index) of A'A, formed
 * in double from the float A, after cvp_sweeps_tri() sweeps of cvp_jacobi, rounded to float */
void cvp_null4(const float *A, float *e);
/* cv::Mat::inv() of a 3 x 3 float matrix (LocalMapping.cc:653): determinant and cofactors in double, times 1 / det, rounded to float;
 * the zero matrix where the determinant is zero */
void cvp_inv3f(const float *S, float *D);
/* the sweep count of cvp_null4, read from sivo_amd/csrc/triangulate_math.hpp */
int cvp_sweeps_tri(void);
#ifdef __cplusplus
}
#endif
