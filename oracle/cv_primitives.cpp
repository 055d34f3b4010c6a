// See cv_primitives.h.  Only + - * / sqrt, comparisons and float / double conversions; compiled with -ffp-contract=off.
#include "cv_primitives.h"

#include <cmath>
#include <limits>

#ifndef CVP_SWEEPS3
#error "CVP_SWEEPS3 / CVP_SWEEPS12 / CVP_SWEEPS_SVD / CVP_SWEEPS4 come from the kernels' sources (oracle/Makefile)"
#endif
#ifndef CVP_SWEEPS_TRI
#error "CVP_SWEEPS_TRI comes from sivo_amd/csrc/triangulate_math.hpp (oracle/Makefile)"
#endif

namespace {
// the rotation that annihilates the off-diagonal entry `off` between diagonal entries lo (index p) and hi (index q): tangent,
// cosine, sine of the smaller angle
inline void rotation(double lo, double hi, double off, double &t, double &c, double &s) {
    const double theta = (hi - lo) / (2.0 * off);
    t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    c = 1.0 / std::sqrt(t * t + 1.0);
    s = t * c;
}
}  // namespace

extern "C" {

void cvp_sweeps(int *out4) { out4[0] = CVP_SWEEPS3; out4[1] = CVP_SWEEPS12; out4[2] = CVP_SWEEPS_SVD; out4[3] = CVP_SWEEPS4; }

void cvp_mul_transposed(const double *src, int rows, int cols, double *dst) {
    for (int a = 0; a < cols; ++a)
        for (int b = 0; b < cols; ++b) {
            double s = 0.0;
            for (int i = 0; i < rows; ++i) s = s + src[i * cols + a] * src[i * cols + b];
            dst[a * cols + b] = s;
        }
}

void cvp_jacobi(double *A, double *V, int m, int sweeps) {
    for (int sweep = 0; sweep < sweeps; ++sweep)
        for (int p = 0; p < m - 1; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = A[p * m + q], app = A[p * m + p], aqq = A[q * m + q];
                if (!(apq != 0.0)) continue;
                double t, c, s;
                rotation(app, aqq, apq, t, c, s);
                for (int r = 0; r < m; ++r) {
                    if (r == p || r == q) continue;
                    const double arp = A[r * m + p], arq = A[r * m + q];
                    A[r * m + p] = A[p * m + r] = c * arp - s * arq;
                    A[r * m + q] = A[q * m + r] = s * arp + c * arq;
                }
                A[p * m + p] = app - t * apq;
                A[q * m + q] = aqq + t * apq;
                A[p * m + q] = A[q * m + p] = 0.0;
                for (int r = 0; r < m; ++r) {
                    const double vrp = V[r * m + p], vrq = V[r * m + q];
                    V[r * m + p] = c * vrp - s * vrq;
                    V[r * m + q] = s * vrp + c * vrq;
                }
            }
}

void cvp_order(const double *d, int m, int *order) {
    bool used[16] = {false};
    for (int k = 0; k < m; ++k) {
        int best = -1;
        for (int j = 0; j < m; ++j)
            if (!used[j] && (best < 0 || std::fabs(d[j]) > std::fabs(d[best]))) best = j;
        order[k] = best;
        used[best] = true;
    }
}

void cvp_svd_symmetric(double *A, int m, double *W, double *Ut) {
    double V[144], d[12];
    int order[12];
    for (int i = 0; i < m * m; ++i) V[i] = (i / m == i % m) ? 1.0 : 0.0;
    cvp_jacobi(A, V, m, m == 3 ? CVP_SWEEPS3 : CVP_SWEEPS12);
    for (int i = 0; i < m; ++i) d[i] = A[i * m + i];
    cvp_order(d, m, order);
    for (int k = 0; k < m; ++k) {
        W[k] = d[order[k]];
        for (int r = 0; r < m; ++r) Ut[k * m + r] = V[r * m + order[k]];
    }
}

void cvp_svd3(double *A, double *W, double *U, double *V) {
    for (int i = 0; i < 9; ++i) V[i] = (i / 3 == i % 3) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < CVP_SWEEPS_SVD; ++sweep)
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double alpha = A[p] * A[p] + A[3 + p] * A[3 + p] + A[6 + p] * A[6 + p];
                const double beta = A[q] * A[q] + A[3 + q] * A[3 + q] + A[6 + q] * A[6 + q];
                const double gamma = A[p] * A[q] + A[3 + p] * A[3 + q] + A[6 + p] * A[6 + q];
                if (!(gamma != 0.0)) continue;
                double t, c, s;
                rotation(alpha, beta, gamma, t, c, s);
                for (int r = 0; r < 3; ++r) {
                    const double ap = A[3 * r + p], aq = A[3 * r + q];
                    A[3 * r + p] = c * ap - s * aq;
                    A[3 * r + q] = s * ap + c * aq;
                    const double vp = V[3 * r + p], vq = V[3 * r + q];
                    V[3 * r + p] = c * vp - s * vq;
                    V[3 * r + q] = s * vp + c * vq;
                }
            }
    for (int k = 0; k < 3; ++k) {
        W[k] = std::sqrt(A[k] * A[k] + A[3 + k] * A[3 + k] + A[6 + k] * A[6 + k]);
        for (int r = 0; r < 3; ++r) U[3 * r + k] = A[3 * r + k] / W[k];
    }
}

void cvp_solve(const double *A_in, int nr, int nc, const double *b_in, double *x) {
    double A[64], b[8], A1[8], A2[8];
    for (int i = 0; i < nr * nc; ++i) A[i] = A_in[i];
    for (int i = 0; i < nr; ++i) b[i] = b_in[i];
    for (int k = 0; k < nc; ++k) {
        double eta = std::fabs(A[k * nc + k]);
        for (int i = k + 1; i < nr; ++i) {            // (the reference reads the row behind its counter: rows k .. nr-2)
            const double elt = std::fabs(A[(i - 1) * nc + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0) {
            for (int i = 0; i < nc; ++i) x[i] = std::numeric_limits<double>::quiet_NaN();
            return;
        }
        const double inv_eta = 1. / eta;
        double sum = 0.0;
        for (int i = k; i < nr; ++i) {
            A[i * nc + k] = A[i * nc + k] * inv_eta;
            sum = sum + A[i * nc + k] * A[i * nc + k];
        }
        double sigma = std::sqrt(sum);
        if (A[k * nc + k] < 0) sigma = -sigma;
        A[k * nc + k] = A[k * nc + k] + sigma;
        A1[k] = sigma * A[k * nc + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            double dot = 0;
            for (int i = k; i < nr; ++i) dot = dot + A[i * nc + k] * A[i * nc + j];
            const double tau = dot / A1[k];
            for (int i = k; i < nr; ++i) A[i * nc + j] = A[i * nc + j] - tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; ++j) {                    // b <- Q' b
        double tau = 0;
        for (int i = j; i < nr; ++i) tau = tau + A[i * nc + j] * b[i];
        tau = tau / A1[j];
        for (int i = j; i < nr; ++i) b[i] = b[i] - tau * A[i * nc + j];
    }
    x[nc - 1] = b[nc - 1] / A2[nc - 1];               // x = R^-1 b
    for (int i = nc - 2; i >= 0; --i) {
        double sum = 0;
        for (int j = i + 1; j < nc; ++j) sum = sum + A[i * nc + j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
    }
}

void cvp_invert3(const double *c, double *ci) {
    const double c00 = c[4] * c[8] - c[5] * c[7], c01 = c[5] * c[6] - c[3] * c[8], c02 = c[3] * c[7] - c[4] * c[6];
    const double det = c[0] * c00 + c[1] * c01 + c[2] * c02;
    ci[0] = c00 / det;
    ci[1] = (c[2] * c[7] - c[1] * c[8]) / det;
    ci[2] = (c[1] * c[5] - c[2] * c[4]) / det;
    ci[3] = c01 / det;
    ci[4] = (c[0] * c[8] - c[2] * c[6]) / det;
    ci[5] = (c[2] * c[3] - c[0] * c[5]) / det;
    ci[6] = c02 / det;
    ci[7] = (c[1] * c[6] - c[0] * c[7]) / det;
    ci[8] = (c[0] * c[4] - c[1] * c[3]) / det;
}

void cvp_eigen4(const float *N, float *eval, float *evec) {
    double A[16], V[16];
    for (int i = 0; i < 16; ++i) { A[i] = (double)N[i]; V[i] = (i / 4 == i % 4) ? 1.0 : 0.0; }
    cvp_jacobi(A, V, 4, CVP_SWEEPS4);
    bool used[4] = {false, false, false, false};
    for (int k = 0; k < 4; ++k) {
        int best = -1;
        for (int j = 0; j < 4; ++j)
            if (!used[j] && (best < 0 || A[5 * j] > A[5 * best])) best = j;
        used[best] = true;
        eval[k] = (float)A[5 * best];
        for (int r = 0; r < 4; ++r) evec[4 * k + r] = (float)V[4 * r + best];
    }
}

void cvp_quaternion_rotation(const float *q, float *R) {
    const double w = (double)q[0], x = (double)q[1], y = (double)q[2], z = (double)q[3];
    const double xx = x * x, yy = y * y, zz = z * z, ww = w * w;
    const double v2 = xx + yy + zz;
    const double n2 = ww + v2;
    const double f = v2 / v2;
    R[0] = (float)((ww + xx - yy - zz) / n2 * f);
    R[1] = (float)(2.0 * (x * y - w * z) / n2 * f);
    R[2] = (float)(2.0 * (x * z + w * y) / n2 * f);
    R[3] = (float)(2.0 * (x * y + w * z) / n2 * f);
    R[4] = (float)((ww - xx + yy - zz) / n2 * f);
    R[5] = (float)(2.0 * (y * z - w * x) / n2 * f);
    R[6] = (float)(2.0 * (x * z - w * y) / n2 * f);
    R[7] = (float)(2.0 * (y * z + w * x) / n2 * f);
    R[8] = (float)((ww - xx - yy + zz) / n2 * f);
}

int cvp_sweeps_tri(void) { return CVP_SWEEPS_TRI; }

void cvp_null4(const float *Af, float *e) {
    double A[16], V[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s = s + (double)Af[4 * k + i] * (double)Af[4 * k + j];
            A[4 * i + j] = s;
            V[4 * i + j] = i == j ? 1.0 : 0.0;
        }
    cvp_jacobi(A, V, 4, CVP_SWEEPS_TRI);
    int best = 0;
    for (int j = 1; j < 4; ++j)
        if (A[5 * j] < A[5 * best]) best = j;
    for (int r = 0; r < 4; ++r) e[r] = (float)V[4 * r + best];
}

void cvp_inv3f(const float *S, float *D) {
    double s[9];
    for (int i = 0; i < 9; ++i) { s[i] = (double)S[i]; D[i] = 0.0f; }
    const double m00 = s[4] * s[8] - s[5] * s[7], m01 = s[3] * s[8] - s[5] * s[6], m02 = s[3] * s[7] - s[4] * s[6];
    double d = s[0] * m00 - s[1] * m01 + s[2] * m02;
    if (d == 0.) return;
    d = 1. / d;
    D[0] = (float)(m00 * d);
    D[1] = (float)((s[2] * s[7] - s[1] * s[8]) * d);
    D[2] = (float)((s[1] * s[5] - s[2] * s[4]) * d);
    D[3] = (float)((s[5] * s[6] - s[3] * s[8]) * d);
    D[4] = (float)((s[0] * s[8] - s[2] * s[6]) * d);
    D[5] = (float)((s[2] * s[3] - s[0] * s[5]) * d);
    D[6] = (float)(m02 * d);
    D[7] = (float)((s[1] * s[6] - s[0] * s[7]) * d);
    D[8] = (float)((s[0] * s[4] - s[1] * s[3]) * d);
}

}  // extern "C"
