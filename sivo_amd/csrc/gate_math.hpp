// gate_math.hpp — the mutual information of SIVO's selection gate for ONE keypoint: the body the entropy-gate kernel (select.hip) and the
// triangulation kernel (triangulate.hip, the CheckSemantics call of LocalMapping::CreateNewMapPoints) share.  Stands behind
//   SIVO::computeStereoJacobianPose / computeStereoCovariance / computeStereoMutualInformation
//   (reference src/sivo_helpers/sivo_helpers.cpp:64-88, 160-180, 201-219).
// fp64, determinants as Eigen takes them (3x3 cofactors, 6x6 / 9x9 partial-pivot LU).  Compiles for the device and, with g++, for the
// host (the restatement tests build it into a program of their own).
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

// diagonal().prod() in the order of Eigen's unrolled reduction (halves, recursively), written out for the two sizes used
SIVO_HD double diag_product(const double *d, int n) {
    if (n == 6) return (d[0] * (d[1] * d[2])) * (d[3] * (d[4] * d[5]));
    return ((d[0] * d[1]) * (d[2] * d[3])) * ((d[4] * d[5]) * (d[6] * (d[7] * d[8])));     // n == 9
}

// Eigen::PartialPivLU::determinant (what Matrix<double, 6, 6> / <9, 9>::determinant() evaluates: sivo_helpers.cpp:207-216)
SIVO_HD double det_lu(double *a, int n) {
    double diag[9];
    double sign = 1.0;
    for (int k = 0; k < n; ++k) {
        int piv = k;
        double best = fabs(a[k * n + k]);
        for (int i = k + 1; i < n; ++i)
            if (fabs(a[i * n + k]) > best) { best = fabs(a[i * n + k]); piv = i; }
        if (best == 0.0) return 0.0;
        if (piv != k) {
            for (int j = 0; j < n; ++j) { const double t = a[k * n + j]; a[k * n + j] = a[piv * n + j]; a[piv * n + j] = t; }
            sign = -sign;
        }
        diag[k] = a[k * n + k];
        for (int i = k + 1; i < n; ++i) {
            const double f = a[i * n + k] / a[k * n + k];
            for (int j = k + 1; j < n; ++j) a[i * n + j] -= f * a[k * n + j];
        }
    }
    return sign * diag_product(diag, n);
}

// MI = 0.5 log2(det Sx * det Sz / det S9) of the point (X, Y, Z) against the 6 x 6 state covariance Sx (row-major), measurement noise sigma2 I
SIVO_HD double gate_mutual_information(const double *Sx, double fx, double fy, double bl, double X, double Y, double Z, double sigma2) {
    double J[18];
    for (int k = 0; k < 18; ++k) J[k] = 0.0;
    if (Z != 0) {
        J[0] = fx / Z; J[1] = 0.0; J[2] = -fx * X / (Z * Z);
        J[3] = -fx * X * Y / (Z * Z); J[4] = fx * (1.0 + (X * X) / (Z * Z)); J[5] = -fx * Y / Z;
        J[6] = 0.0; J[7] = fy / Z; J[8] = -fy * Y / (Z * Z);
        J[9] = -fy * (1 + (Y * Y) / (Z * Z)); J[10] = fy * X * Y / (Z * Z); J[11] = fy * X / Z;
        J[12] = fx / Z; J[13] = 0.0; J[14] = -fx * (X - bl) / (Z * Z);
        J[15] = -fx * (X - bl) * Y / (Z * Z); J[16] = fx * (1.0 + (X * (X - bl)) / (Z * Z)); J[17] = -fx * Y / Z;
    }
    double S9[81], JS[18], Sz[9], Sxc[36];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 6; ++b) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += J[a * 6 + k] * Sx[k * 6 + b];
            JS[a * 6 + b] = s;
        }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += JS[a * 6 + k] * J[b * 6 + k];
            Sz[a * 3 + b] = s + (a == b ? sigma2 : 0.0);
        }
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) { S9[a * 9 + b] = Sx[a * 6 + b]; Sxc[a * 6 + b] = Sx[a * 6 + b]; }
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 3; ++b) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += Sx[a * 6 + k] * J[b * 6 + k];
            S9[a * 9 + 6 + b] = s;
        }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 6; ++b) S9[(6 + a) * 9 + b] = JS[a * 6 + b];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) S9[(6 + a) * 9 + 6 + b] = Sz[a * 3 + b];
    const double state_det = det_lu(Sxc, 6);
    const double meas_det = Sz[0] * (Sz[4] * Sz[8] - Sz[5] * Sz[7]) - Sz[1] * (Sz[3] * Sz[8] - Sz[5] * Sz[6]) +
                            Sz[2] * (Sz[3] * Sz[7] - Sz[4] * Sz[6]);
    const double cov_det = det_lu(S9, 9);
    return 0.5 * log2(state_det * meas_det / cov_det);
}

}  // namespace sivo
