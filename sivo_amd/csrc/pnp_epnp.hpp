// pnp_epnp.hpp — the arithmetic of pnp_ransac.hip: EPnP as the reference's PnPsolver states it (src/orbslam/PnPsolver.cc: compute_pose,
// :482-531, and everything it calls) and CheckInliers (:318-347), restated in double operation for operation.  The functions are written
// for a TEAM of lanes that share one PnpWork: every reduction over the n correspondences has one lane per output entry, which sums
// i = 0 .. n-1 in order; every rotation of a Jacobi has one lane per row; the small dense algebra in between (qr_solve, gauss_newton, the
// 3 x 3 SVD) runs on lane 0 over the shared arrays.  No result depends on the team's size: a team of one (PnpHostTeam, a plain g++ build,
// tests/pnp_ransac_prog.cpp) computes the same bits as a wave (PnpWaveTeam in pnp_ransac.hip).  Nothing is kept per point: alphas and
// pcs are recomputed from the control points wherever the reference reads them (the same operations on the same values).
//
// Only + - * / sqrt, comparisons and float / double conversions; compiled without contraction.  OpenCV is absent:
//   cvSVD of the symmetric PW0'PW0 (3 x 3) and M'M (12 x 12)  ->  cyclic Jacobi, PNP_SWEEPS3 / PNP_SWEEPS12 sweeps over the pairs
//       (0,1) (0,2) .. (0,m-1) (1,2) .., a rotation skipped when its off-diagonal entry is exactly zero; eigenpairs ordered by
//       |eigenvalue| descending, ties to the lower index (the order `ut` rows 11, 10, 9, 8 assume);
//   cvMulTransposed  ->  the sum over the rows in order, from 0.0;
//   cvSVD of ABt with U and V  ->  one-sided Jacobi (Hestenes), PNP_SWEEPS_SVD sweeps over the column pairs (0,1) (0,2) (1,2),
//       U = the rotated columns over their norms (a zero norm gives 0 / 0: NaN), singular values left unordered (R = U V' does not
//       depend on their order);
//   cvSolve(CV_SVD) on the 6 x 4 / 6 x 3 / 6 x 5 systems  ->  the reference's own qr_solve (:865-955); where that returns early on an
//       exactly zero column X is NaN;
//   cvInvert(CC, CV_SVD)  ->  adjugate / determinant.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/sivo_hip.h"

#if defined(__HIPCC__)
#define PNP_HD __host__ __device__ inline
#else
#define PNP_HD inline
#endif

namespace sivo {

// (the smallest counts at which two more sweeps change no inlier count of any test scene: DESIGN 3.6d has the measurement)
constexpr int PNP_SWEEPS3 = 4, PNP_SWEEPS12 = 8, PNP_SWEEPS_SVD = 3;

struct PnpHostTeam {
    static constexpr int lane = 0, size = 1;
    void sync() const {}
};

// Everything a team shares (LDS on the device: ~5 KiB)
struct PnpWork {
    double A[144], V[144];            // M'M and its eigenvectors (columns)
    double s3[9], v3[9];              // PW0'PW0 and its eigenvectors
    double cws[4][3], ci[9], rho[6];
    double nv[4][12];                 // v[0..3] = ut rows 11, 10, 9, 8
    double L[60];
    double qa[30], qb[6], qx[5], a1[5], a2[5];
    double betas[4], ccs[4][3], pc0[3], pw0[3], abt[9], w3[9];
    double Rs[3][9], ts[3][3], err[3];
    int32_t ord[12];
};

struct PnpPt { double X, Y, Z, u, v; };

// add_correspondence(:373-383): the floats widen to double
PNP_HD PnpPt pnp_pt(const SivoPnpPoint *pts, const int32_t *idx, int i) {
    const SivoPnpPoint &q = pts[idx[i]];
    return PnpPt{(double)q.xw[0], (double)q.xw[1], (double)q.xw[2], (double)q.u, (double)q.v};
}

PNP_HD double pnp_nan() { return __builtin_nan(""); }

PNP_HD double pnp_dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// one row of alphas (:431-440)
PNP_HD void pnp_alphas(const PnpWork &w, const PnpPt &p, double &a0, double &a1, double &a2, double &a3) {
    const double d0 = p.X - w.cws[0][0], d1 = p.Y - w.cws[0][1], d2 = p.Z - w.cws[0][2];
    a1 = w.ci[0] * d0 + w.ci[1] * d1 + w.ci[2] * d2;
    a2 = w.ci[3] * d0 + w.ci[4] * d1 + w.ci[5] * d2;
    a3 = w.ci[6] * d0 + w.ci[7] * d1 + w.ci[8] * d2;
    a0 = 1.0 - a1 - a2 - a3;
}

// one coordinate of pcs (:471-480)
PNP_HD double pnp_pc(const PnpWork &w, double a0, double a1, double a2, double a3, int j) {
    return a0 * w.ccs[0][j] + a1 * w.ccs[1][j] + a2 * w.ccs[2][j] + a3 * w.ccs[3][j];
}

// Cyclic Jacobi of the symmetric m x m matrix A (row-major, both halves kept), V = the accumulated rotations.  Every lane forms the
// rotation from the same three entries; lane r then rotates row r of A (and its mirror) and of V.
template <class Team>
PNP_HD void pnp_jacobi(const Team &T, double *A, double *V, int m, int sweeps) {
    for (int sweep = 0; sweep < sweeps; ++sweep)
        for (int p = 0; p < m - 1; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = A[p * m + q], app = A[p * m + p], aqq = A[q * m + q];
                T.sync();
                if (apq != 0.0) {      // (a NaN enters: it propagates as every other value does)
                    const double theta = (aqq - app) / (2.0 * apq);
                    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                    const double c = 1.0 / sqrt(t * t + 1.0);
                    const double s = t * c;
                    for (int r = T.lane; r < m; r += T.size) {
                        if (r == p) {
                            A[p * m + p] = app - t * apq;
                            A[q * m + q] = aqq + t * apq;
                            A[p * m + q] = 0.0; A[q * m + p] = 0.0;
                        } else if (r != q) {
                            const double arp = A[r * m + p], arq = A[r * m + q];
                            const double np_ = c * arp - s * arq, nq_ = s * arp + c * arq;
                            A[r * m + p] = np_; A[p * m + r] = np_;
                            A[r * m + q] = nq_; A[q * m + r] = nq_;
                        }
                        const double vrp = V[r * m + p], vrq = V[r * m + q];
                        V[r * m + p] = c * vrp - s * vrq;
                        V[r * m + q] = s * vrp + c * vrq;
                    }
                }
                T.sync();
            }
}

// ord[k] = the index of the k-th largest |A[i][i]|, ties (and everything that does not compare) to the lower index
PNP_HD void pnp_order(const double *A, int m, int32_t *ord) {
    uint32_t used = 0;
    for (int k = 0; k < m; ++k) {
        int best = -1;
        for (int j = 0; j < m; ++j) {
            if (used >> j & 1) continue;
            if (best < 0 || fabs(A[j * m + j]) > fabs(A[best * m + best])) best = j;
        }
        ord[k] = best;
        used |= 1u << best;
    }
}

// qr_solve (:865-955) on the nr x nc system A X = b (A and b are overwritten).  The reference's scan for the largest element of a
// column reads one row behind its counter: it sees rows k .. nr-2, as here.
PNP_HD void pnp_qr_solve(double *A, double *b, double *X, double *A1, double *A2, int nr, int nc) {
    for (int k = 0; k < nc; ++k) {
        double eta = fabs(A[k * nc + k]);
        for (int i = k + 1; i < nr; ++i) {
            const double elt = fabs(A[(i - 1) * nc + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0) {                // (the reference returns with X unset)
            for (int i = 0; i < nc; ++i) X[i] = pnp_nan();
            return;
        }
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        for (int i = k; i < nr; ++i) {
            A[i * nc + k] = A[i * nc + k] * inv_eta;
            sum = sum + A[i * nc + k] * A[i * nc + k];
        }
        double sigma = sqrt(sum);
        if (A[k * nc + k] < 0) sigma = -sigma;
        A[k * nc + k] = A[k * nc + k] + sigma;
        A1[k] = sigma * A[k * nc + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            double s = 0;
            for (int i = k; i < nr; ++i) s = s + A[i * nc + k] * A[i * nc + j];
            const double tau = s / A1[k];
            for (int i = k; i < nr; ++i) A[i * nc + j] = A[i * nc + j] - tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; ++j) {     // b <- Qt b
        double tau = 0;
        for (int i = j; i < nr; ++i) tau = tau + A[i * nc + j] * b[i];
        tau = tau / A1[j];
        for (int i = j; i < nr; ++i) b[i] = b[i] - tau * A[i * nc + j];
    }
    X[nc - 1] = b[nc - 1] / A2[nc - 1];  // X = R-1 b
    for (int i = nc - 2; i >= 0; --i) {
        double s = 0;
        for (int j = i + 1; j < nc; ++j) s = s + A[i * nc + j] * X[j];
        X[i] = (b[i] - s) / A2[i];
    }
}

// find_betas_approx_1 / _2 / _3 (:669-762), kind = 1, 2, 3; cvSolve is qr_solve on a copy
PNP_HD void pnp_find_betas(PnpWork &w, int kind) {
    const int nc = kind == 1 ? 4 : kind == 2 ? 3 : 5;
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < nc; ++j) {
            const int col = kind == 1 ? (j == 0 ? 0 : j == 1 ? 1 : j == 2 ? 3 : 6) : j;
            w.qa[i * nc + j] = w.L[10 * i + col];
        }
        w.qb[i] = w.rho[i];
    }
    pnp_qr_solve(w.qa, w.qb, w.qx, w.a1, w.a2, 6, nc);
    const double *b = w.qx;
    double *betas = w.betas;
    if (kind == 1) {
        if (b[0] < 0) {
            betas[0] = sqrt(-b[0]);
            betas[1] = -b[1] / betas[0]; betas[2] = -b[2] / betas[0]; betas[3] = -b[3] / betas[0];
        } else {
            betas[0] = sqrt(b[0]);
            betas[1] = b[1] / betas[0]; betas[2] = b[2] / betas[0]; betas[3] = b[3] / betas[0];
        }
        return;
    }
    if (b[0] < 0) {
        betas[0] = sqrt(-b[0]);
        betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
    } else {
        betas[0] = sqrt(b[0]);
        betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
    }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = kind == 3 ? b[3] / betas[0] : 0.0;
    betas[3] = 0.0;
}

// gauss_newton (:845-863) with compute_A_and_b_gauss_newton (:814-843)
PNP_HD void pnp_gauss_newton(PnpWork &w) {
    double *be = w.betas;
    for (int k = 0; k < 5; ++k) {
        for (int i = 0; i < 6; ++i) {
            const double *l = w.L + 10 * i;
            double *a = w.qa + 4 * i;
            a[0] = 2 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3];
            a[1] = l[1] * be[0] + 2 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3];
            a[2] = l[3] * be[0] + l[4] * be[1] + 2 * l[5] * be[2] + l[8] * be[3];
            a[3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2 * l[9] * be[3];
            w.qb[i] = w.rho[i] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] +
                                  l[4] * be[1] * be[2] + l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] +
                                  l[8] * be[2] * be[3] + l[9] * be[3] * be[3]);
        }
        pnp_qr_solve(w.qa, w.qb, w.qx, w.a1, w.a2, 6, 4);
        for (int i = 0; i < 4; ++i) be[i] = be[i] + w.qx[i];
    }
}

// cvSVD(ABt, D, U, V) by one-sided Jacobi, then R = U V' with the det < 0 flip and t (:610-629).  G = w.abt is rotated in place.
PNP_HD void pnp_rotation(PnpWork &w, double *R, double *t) {
    double *G = w.abt, *W = w.w3;
    for (int i = 0; i < 9; ++i) W[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < PNP_SWEEPS_SVD; ++sweep)
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double alpha = G[p] * G[p] + G[3 + p] * G[3 + p] + G[6 + p] * G[6 + p];
                const double beta = G[q] * G[q] + G[3 + q] * G[3 + q] + G[6 + q] * G[6 + q];
                const double gamma = G[p] * G[q] + G[3 + p] * G[3 + q] + G[6 + p] * G[6 + q];
                if (gamma != 0.0) {
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    double tt = 1.0 / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
                    if (zeta < 0.0) tt = -tt;
                    const double c = 1.0 / sqrt(tt * tt + 1.0);
                    const double s = tt * c;
                    for (int r = 0; r < 3; ++r) {
                        const double gp = G[3 * r + p], gq = G[3 * r + q];
                        G[3 * r + p] = c * gp - s * gq;
                        G[3 * r + q] = s * gp + c * gq;
                        const double wp = W[3 * r + p], wq = W[3 * r + q];
                        W[3 * r + p] = c * wp - s * wq;
                        W[3 * r + q] = s * wp + c * wq;
                    }
                }
            }
    for (int k = 0; k < 3; ++k) {      // U = the columns over their norms
        const double sigma = sqrt(G[k] * G[k] + G[3 + k] * G[3 + k] + G[6 + k] * G[6 + k]);
        for (int r = 0; r < 3; ++r) G[3 * r + k] = G[3 * r + k] / sigma;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = pnp_dot3(G + 3 * i, W + 3 * j);
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] -
                       R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
    for (int i = 0; i < 3; ++i) t[i] = w.pc0[i] - pnp_dot3(R + 3 * i, w.pw0);
}

// compute_pose (:482-531) on the n >= 4 correspondences pts[idx[0 .. n-1]], K = fu fv uc vc.  Returns which of Rs / ts holds the pose
// (every lane returns the same value; the caller reads w after the call).
template <class Team>
PNP_HD int pnp_epnp(const Team &T, PnpWork &w, const SivoPnpPoint *pts, const int32_t *idx, int n, const double (&K)[4]) {
    const double fu = K[0], fv = K[1], uc = K[2], vc = K[3];
    // choose_control_points (:385-418)
    for (int e = T.lane; e < 3; e += T.size) {
        double s = 0;
        for (int i = 0; i < n; ++i) {
            const PnpPt p = pnp_pt(pts, idx, i);
            s = s + (e == 0 ? p.X : e == 1 ? p.Y : p.Z);
        }
        w.cws[0][e] = s / n;
    }
    T.sync();
    for (int e = T.lane; e < 9; e += T.size) {
        const int a = e / 3, b = e % 3;
        w.v3[e] = a == b ? 1.0 : 0.0;
        if (a > b) continue;
        double s = 0.0;
        for (int i = 0; i < n; ++i) {
            const PnpPt p = pnp_pt(pts, idx, i);
            const double da = (a == 0 ? p.X : a == 1 ? p.Y : p.Z) - w.cws[0][a];
            const double db = (b == 0 ? p.X : b == 1 ? p.Y : p.Z) - w.cws[0][b];
            s = s + da * db;
        }
        w.s3[3 * a + b] = s; w.s3[3 * b + a] = s;
    }
    T.sync();
    pnp_jacobi(T, w.s3, w.v3, 3, PNP_SWEEPS3);
    if (T.lane == 0) {
        pnp_order(w.s3, 3, w.ord);
        for (int i = 1; i < 4; ++i) {
            const int o = w.ord[i - 1];
            const double k = sqrt(w.s3[4 * o] / n);
            for (int j = 0; j < 3; ++j) w.cws[i][j] = w.cws[0][j] + k * w.v3[3 * j + o];
        }
        // compute_barycentric_coordinates (:420-429): CC and its inverse
        double cc[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 1; j < 4; ++j) cc[3 * i + j - 1] = w.cws[j][i] - w.cws[0][i];
        const double c00 = cc[4] * cc[8] - cc[5] * cc[7], c01 = cc[5] * cc[6] - cc[3] * cc[8], c02 = cc[3] * cc[7] - cc[4] * cc[6];
        const double det = cc[0] * c00 + cc[1] * c01 + cc[2] * c02;
        w.ci[0] = c00 / det; w.ci[1] = (cc[2] * cc[7] - cc[1] * cc[8]) / det; w.ci[2] = (cc[1] * cc[5] - cc[2] * cc[4]) / det;
        w.ci[3] = c01 / det; w.ci[4] = (cc[0] * cc[8] - cc[2] * cc[6]) / det; w.ci[5] = (cc[2] * cc[3] - cc[0] * cc[5]) / det;
        w.ci[6] = c02 / det; w.ci[7] = (cc[1] * cc[6] - cc[0] * cc[7]) / det; w.ci[8] = (cc[0] * cc[4] - cc[1] * cc[3]) / det;
        // compute_rho (:805-812)
        int r = 0;
        for (int a = 0; a < 3; ++a)
            for (int b = a + 1; b < 4; ++b) {
                const double *p1 = w.cws[a], *p2 = w.cws[b];
                w.rho[r++] = (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
            }
    }
    T.sync();
    // fill_M (:443-457) and M'M: entry (p, q), p <= q, is the sum over the rows 0 .. 2n-1 in order
    for (int e = T.lane; e < 144; e += T.size) w.V[e] = (e % 13 == 0) ? 1.0 : 0.0;
    for (int e = T.lane; e < 78; e += T.size) {
        int p = 0, rem = e;
        while (rem >= 12 - p) { rem -= 12 - p; ++p; }
        const int q = p + rem, ip = p / 3, kp = p % 3, iq = q / 3, kq = q % 3;
        double s = 0.0;
        for (int i = 0; i < n; ++i) {
            const PnpPt pt = pnp_pt(pts, idx, i);
            double a0, a1, a2, a3;
            pnp_alphas(w, pt, a0, a1, a2, a3);
            const double ap = ip == 0 ? a0 : ip == 1 ? a1 : ip == 2 ? a2 : a3;
            const double aq = iq == 0 ? a0 : iq == 1 ? a1 : iq == 2 ? a2 : a3;
            const double du = uc - pt.u, dv = vc - pt.v;
            const double m1p = kp == 0 ? ap * fu : kp == 1 ? 0.0 : ap * du, m1q = kq == 0 ? aq * fu : kq == 1 ? 0.0 : aq * du;
            const double m2p = kp == 0 ? 0.0 : kp == 1 ? ap * fv : ap * dv, m2q = kq == 0 ? 0.0 : kq == 1 ? aq * fv : aq * dv;
            s = s + m1p * m1q;
            s = s + m2p * m2q;
        }
        w.A[12 * p + q] = s; w.A[12 * q + p] = s;
    }
    T.sync();
    pnp_jacobi(T, w.A, w.V, 12, PNP_SWEEPS12);
    if (T.lane == 0) {
        pnp_order(w.A, 12, w.ord);
        for (int i = 0; i < 4; ++i)
            for (int c = 0; c < 12; ++c) w.nv[i][c] = w.V[12 * c + w.ord[11 - i]];
        // compute_L_6x10 (:764-803)
        int a = 0, b = 1;
        for (int j = 0; j < 6; ++j) {
            double dv[4][3];
            for (int i = 0; i < 4; ++i)
                for (int k = 0; k < 3; ++k) dv[i][k] = w.nv[i][3 * a + k] - w.nv[i][3 * b + k];
            double *row = w.L + 10 * j;
            row[0] = pnp_dot3(dv[0], dv[0]);
            row[1] = 2.0 * pnp_dot3(dv[0], dv[1]);
            row[2] = pnp_dot3(dv[1], dv[1]);
            row[3] = 2.0 * pnp_dot3(dv[0], dv[2]);
            row[4] = 2.0 * pnp_dot3(dv[1], dv[2]);
            row[5] = pnp_dot3(dv[2], dv[2]);
            row[6] = 2.0 * pnp_dot3(dv[0], dv[3]);
            row[7] = 2.0 * pnp_dot3(dv[1], dv[3]);
            row[8] = 2.0 * pnp_dot3(dv[2], dv[3]);
            row[9] = pnp_dot3(dv[3], dv[3]);
            b++;
            if (b > 3) { a++; b = a + 1; }
        }
    }
    T.sync();
    for (int sol = 0; sol < 3; ++sol) {
        if (T.lane == 0) {
            pnp_find_betas(w, sol + 1);
            pnp_gauss_newton(w);
            // compute_ccs (:459-469), compute_pcs of the first point, solve_for_sign (:638-650): the pcs of a negated ccs are the
            // negated pcs
            for (int j = 0; j < 4; ++j)
                for (int k = 0; k < 3; ++k) {
                    double s = 0.0;
                    for (int i = 0; i < 4; ++i) s = s + w.betas[i] * w.nv[i][3 * j + k];
                    w.ccs[j][k] = s;
                }
            double a0, a1, a2, a3;
            pnp_alphas(w, pnp_pt(pts, idx, 0), a0, a1, a2, a3);
            if (pnp_pc(w, a0, a1, a2, a3, 2) < 0.0)
                for (int j = 0; j < 4; ++j)
                    for (int k = 0; k < 3; ++k) w.ccs[j][k] = -w.ccs[j][k];
        }
        T.sync();
        // estimate_R_and_t (:572-630)
        for (int e = T.lane; e < 6; e += T.size) {
            double s = 0.0;
            for (int i = 0; i < n; ++i) {
                const PnpPt pt = pnp_pt(pts, idx, i);
                if (e < 3) {
                    double a0, a1, a2, a3;
                    pnp_alphas(w, pt, a0, a1, a2, a3);
                    s = s + pnp_pc(w, a0, a1, a2, a3, e);
                } else {
                    s = s + (e == 3 ? pt.X : e == 4 ? pt.Y : pt.Z);
                }
            }
            if (e < 3) w.pc0[e] = s / n; else w.pw0[e - 3] = s / n;
        }
        T.sync();
        for (int e = T.lane; e < 9; e += T.size) {
            const int j = e / 3, k = e % 3;
            double s = 0.0;
            for (int i = 0; i < n; ++i) {
                const PnpPt pt = pnp_pt(pts, idx, i);
                double a0, a1, a2, a3;
                pnp_alphas(w, pt, a0, a1, a2, a3);
                const double pc = pnp_pc(w, a0, a1, a2, a3, j);
                const double pw = k == 0 ? pt.X : k == 1 ? pt.Y : pt.Z;
                s = s + (pc - w.pc0[j]) * (pw - w.pw0[k]);
            }
            w.abt[e] = s;
        }
        T.sync();
        if (T.lane == 0) {
            double *R = w.Rs[sol], *t = w.ts[sol];
            pnp_rotation(w, R, t);
            // reprojection_error (:554-570)
            double sum2 = 0.0;
            for (int i = 0; i < n; ++i) {
                const PnpPt pt = pnp_pt(pts, idx, i);
                const double pw[3] = {pt.X, pt.Y, pt.Z};
                const double Xc = pnp_dot3(R, pw) + t[0];
                const double Yc = pnp_dot3(R + 3, pw) + t[1];
                const double inv_Zc = 1.0 / (pnp_dot3(R + 6, pw) + t[2]);
                const double ue = uc + fu * Xc * inv_Zc;
                const double ve = vc + fv * Yc * inv_Zc;
                sum2 = sum2 + sqrt((pt.u - ue) * (pt.u - ue) + (pt.v - ve) * (pt.v - ve));
            }
            w.err[sol] = sum2 / n;
        }
        T.sync();
    }
    int N = 0;
    if (w.err[1] < w.err[0]) N = 1;
    if (w.err[2] < w.err[N]) N = 2;
    return N;
}

// CheckInliers (:318-347) for one correspondence, with the source's own mixture: Xc, Yc, invZc are double expressions narrowed to
// float, ue / ve double, the distances and error2 float, the comparison float.  A NaN error is not an inlier.
PNP_HD bool pnp_inlier(const double *R, const double *t, const double (&K)[4], float X, float Y, float Z, float u, float v, float max_err) {
    const float Xc = (float)(R[0] * X + R[1] * Y + R[2] * Z + t[0]);
    const float Yc = (float)(R[3] * X + R[4] * Y + R[5] * Z + t[1]);
    const float invZc = (float)(1 / (R[6] * X + R[7] * Y + R[8] * Z + t[2]));
    const double ue = K[2] + K[0] * Xc * invZc;
    const double ve = K[3] + K[1] * Yc * invZc;
    const float distX = (float)(u - ue);
    const float distY = (float)(v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_err;
}

}  // namespace sivo
