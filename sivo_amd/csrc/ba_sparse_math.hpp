// ba_sparse_math.hpp — the per-block bodies of the sparse reduced camera system of the bundle adjustment (ba_solve.hip):
// one entry of a Schur contribution, the 6 x 6 Cholesky with reciprocal pivots, one row of a panel solve, the 6-term products of the
// update lists and of the triangular solves.  The kernels give one lane one entry of a block and call these; compiled by g++, the host
// program of the tests (tests/ba_sparse_host_capi.hpp) walks the same blocks in sequence through the same code.  fp64, no contraction
// (the including file sets it), every sum in a fixed order.
#pragma once
#include <math.h>

#ifndef SIVO_HD
#ifdef __HIPCC__
#define SIVO_HD __host__ __device__ inline
#else
#define SIVO_HD inline
#endif
#endif

namespace sivo {

// (Hll_q + lambda I)^-1 of a 3 x 3 point block, by cofactors
SIVO_HD void bs_point_inverse(const double *Hll, double lambda, double (&Ai)[9]) {
    double A[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = Hll[i];
    A[0] += lambda; A[4] += lambda; A[8] += lambda;
    const double c0 = A[4] * A[8] - A[5] * A[7], c1 = A[5] * A[6] - A[3] * A[8], c2 = A[3] * A[7] - A[4] * A[6];
    const double det = A[0] * c0 + A[1] * c1 + A[2] * c2, id = 1.0 / det;
    Ai[0] = c0 * id; Ai[1] = (A[2] * A[7] - A[1] * A[8]) * id; Ai[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    Ai[3] = c1 * id; Ai[4] = (A[0] * A[8] - A[2] * A[6]) * id; Ai[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    Ai[6] = c2 * id; Ai[7] = (A[1] * A[6] - A[0] * A[7]) * id; Ai[8] = (A[0] * A[4] - A[1] * A[3]) * id;
}

// row r of Y = W (Hll + lambda I)^-1 from row r of W (3 doubles)
SIVO_HD void bs_y_row(const double *Wr, const double (&Ai)[9], double (&y)[3]) {
#pragma unroll
    for (int b = 0; b < 3; ++b) y[b] = Wr[0] * Ai[b] + Wr[1] * Ai[3 + b] + Wr[2] * Ai[6 + b];
}
// one entry of a contribution: (Y W'^T)[r][c] from row r of Y and row c of W' (or Y bl from bl)
SIVO_HD double bs_contrib(const double (&y)[3], const double *w) { return y[0] * w[0] + y[1] * w[1] + y[2] * w[2]; }

// lower Cholesky factor of the 6 x 6 matrix A (row-major, lower triangle read), the reciprocals of its diagonal in rd; false when a
// pivot is not positive (the factor is then not to be used)
SIVO_HD bool bs_chol6(double (&A)[36], double (&rd)[6]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j * 6 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= A[j * 6 + k] * A[j * 6 + k];
        ok = ok && (d > 0.0);
        d = sqrt(d);
        A[j * 6 + j] = d;
        rd[j] = 1.0 / d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = A[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= A[i * 6 + k] * A[j * 6 + k];
            A[i * 6 + j] = s * rd[j];
        }
    }
    return ok;
}

// one row of the panel solve X L_jj^T = R: X from the row of R, the diagonal block's factor and its reciprocal pivots
SIVO_HD void bs_panel_row(const double (&row)[6], const double *Lj, const double *rj, double (&X)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double s = row[c];
#pragma unroll
        for (int m = 0; m < c; ++m) s -= X[m] * Lj[6 * c + m];
        X[c] = s * rj[c];
    }
}

// the 6-term products of the update lists and the triangular solves: a row of a block times a row of a block (or a vector), and a
// column of a block (stride 6) times a vector
SIVO_HD double bs_dot6(const double *a, const double *b) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 6; ++m) s += a[m] * b[m];
    return s;
}
SIVO_HD double bs_dot6_col(const double *a, const double *x) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 6; ++m) s += a[6 * m] * x[m];
    return s;
}

// y = L_jj^-1 s and x = L_jj^-T s with the reciprocal pivots
SIVO_HD void bs_forward6(const double (&s)[6], const double *Lj, const double *rj, double (&y)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double a = s[i];
#pragma unroll
        for (int m = 0; m < i; ++m) a -= Lj[6 * i + m] * y[m];
        y[i] = a * rj[i];
    }
}
SIVO_HD void bs_backward6(const double (&s)[6], const double *Lj, const double *rj, double (&x)[6]) {
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double a = s[i];
#pragma unroll
        for (int m = i + 1; m < 6; ++m) a -= Lj[6 * m + i] * x[m];
        x[i] = a * rj[i];
    }
}

}  // namespace sivo
