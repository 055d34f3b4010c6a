// sim3_common.hpp — g2o::Sim3 on the device (product, inverse, map, exponential; Eigen's operation order), shared by sim3.hip
// (OptimizeSim3) and essential_graph.hip (OptimizeEssentialGraph).  Moved verbatim from sim3.hip.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace sivo {

// ------------------------------------------------------------------------------------------------
// g2o::Sim3 (types/sim3/sim3.h) — r (Eigen quaternion x y z w), t, s; operation order as Eigen evaluates it
// ------------------------------------------------------------------------------------------------
struct Sim3 { double q[4], t[3], s; };

// Eigen's Quaternion * Vector3 (_transformVector): uv = q.vec x v; uv += uv; v + w uv + q.vec x uv
__device__ __forceinline__ void quat_rotate(const double (&q)[4], const double (&v)[3], double (&o)[3]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    double u0 = y * v[2] - z * v[1], u1 = z * v[0] - x * v[2], u2 = x * v[1] - y * v[0];
    u0 = u0 + u0; u1 = u1 + u1; u2 = u2 + u2;
    o[0] = v[0] + w * u0 + (y * u2 - z * u1);
    o[1] = v[1] + w * u1 + (z * u0 - x * u2);
    o[2] = v[2] + w * u2 + (x * u1 - y * u0);
}

// s * (r * X) + t
__device__ __forceinline__ void sim3_map(const Sim3 &S, const double (&X)[3], double (&Y)[3]) {
    double r[3];
    quat_rotate(S.q, X, r);
#pragma unroll
    for (int i = 0; i < 3; ++i) Y[i] = S.s * r[i] + S.t[i];
}

// Sim3::operator*: r = ra rb, t = sa (ra tb) + ta, s = sa sb
__device__ __forceinline__ Sim3 sim3_mul(const Sim3 &a, const Sim3 &b) {
    Sim3 o;
    const double ax = a.q[0], ay = a.q[1], az = a.q[2], aw = a.q[3], bx = b.q[0], by = b.q[1], bz = b.q[2], bw = b.q[3];
    o.q[0] = aw * bx + ax * bw + ay * bz - az * by;
    o.q[1] = aw * by + ay * bw + az * bx - ax * bz;
    o.q[2] = aw * bz + az * bw + ax * by - ay * bx;
    o.q[3] = aw * bw - ax * bx - ay * by - az * bz;
    double r[3];
    quat_rotate(a.q, b.t, r);
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = a.s * r[i] + a.t[i];
    o.s = a.s * b.s;
    return o;
}

// Sim3::inverse: (r^*, r^* ((-1/s) t), 1/s)
__device__ __forceinline__ Sim3 sim3_inv(const Sim3 &a) {
    Sim3 o;
    o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
    const double f = -1. / a.s;
    const double ft[3] = {f * a.t[0], f * a.t[1], f * a.t[2]};
    double r[3];
    quat_rotate(o.q, ft, r);
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = r[i];
    o.s = 1. / a.s;
    return o;
}

// Sim3(const Vector7d &update), u = [omega, upsilon, sigma], branch by branch (|sigma| < 1e-5, theta < 1e-5), then
// r = Quaterniond(R) (the trace-branch construction; R is not re-orthogonalised in the small-theta branches, nor is r normalised)
__device__ __forceinline__ Sim3 sim3_exp(const double (&u)[7]) {
    const double wx = u[0], wy = u[1], wz = u[2], sigma = u[6];
    const double theta = sqrt(wx * wx + wy * wy + wz * wz);
    const double Om[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    const double s = exp(sigma);
    double Om2[9], R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Om2[3 * i + j] = Om[3 * i] * Om[j] + Om[3 * i + 1] * Om[3 + j] + Om[3 * i + 2] * Om[6 + j];
    const double eps = 0.00001;
    double A, B, C;
    const bool small_theta = theta < eps;
    if (small_theta) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + Om[i] + Om2[i];
    } else {
        const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta);
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * Om[i] + b * Om2[i];
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) {
            A = 1. / 2.; B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sin(theta), b = s * cos(theta), theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    Sim3 o;
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) {
        double t = sqrt(tr + 1.0);
        o.q[3] = 0.5 * t;
        t = 0.5 / t;
        o.q[0] = (R[7] - R[5]) * t; o.q[1] = (R[2] - R[6]) * t; o.q[2] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
        o.q[i] = 0.5 * t;
        t = 0.5 / t;
        o.q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
        o.q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
        o.q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double W0 = A * Om[3 * i] + B * Om2[3 * i] + C * (i == 0 ? 1.0 : 0.0);
        const double W1 = A * Om[3 * i + 1] + B * Om2[3 * i + 1] + C * (i == 1 ? 1.0 : 0.0);
        const double W2 = A * Om[3 * i + 2] + B * Om2[3 * i + 2] + C * (i == 2 ? 1.0 : 0.0);
        o.t[i] = W0 * u[3] + W1 * u[4] + W2 * u[5];
    }
    o.s = s;
    return o;
}

}  // namespace sivo
