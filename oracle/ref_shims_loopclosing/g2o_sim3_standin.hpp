// g2o::Sim3 / g2o::SE3Quat and the Eigen pieces under them for the oracle/_ref build of the reference's LoopClosing.cc (oracle/Makefile,
// ref_loopclosing).  Neither g2o nor Eigen is installed, so this is a SUBSTITUTION, written in the operation order of
// g2o's published types/sim3/sim3.h and Eigen 3.3's Geometry/Quaternion.h — the order sivo_amd/csrc/sim3_common.hpp and
// tests/essential_graph_restatement.py state:
//   * Sim3(R, t, s) keeps r = Quaterniond(R) as the trace-branch construction leaves it: NOT normalised, held as a quaternion;
//   * operator*: r = ra * rb (the quaternion product), t = sa * (ra * tb) + ta, s = sa * sb;
//   * inverse(): (r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s);
//   * map(x): s * (r * x) + t, with r * x Eigen's _transformVector (uv = vec x v; uv += uv; v + w * uv + vec x uv);
//   * rotation() hands the quaternion out; toRotationMatrix() is Eigen's.
// It is NOT the Sim3 of ref_shims_g2o/g2o_standin.hpp, which normalises the quaternion and keeps a rotation matrix (ref_optimizer.o and
// tests/golden/optimizer_reference.txt rest on that one; it is left as it is).  Quaterniond itself is the class of
// ref_shims_g2o/eigen_g2o_ext.hpp; the product, the conjugate and the rotation of a vector are free functions over its accessors here.
// Test infrastructure only.
#pragma once
#include "../ref_shims_g2o/eigen_g2o_ext.hpp"

namespace Eigen {

// QuaternionBase::operator* (internal::quat_product<Architecture::Target, ..., double>)
inline Quaterniond quat_product(const Quaterniond &a, const Quaterniond &b) {
    return Quaterniond(a.w() * b.w() - a.x() * b.x() - a.y() * b.y() - a.z() * b.z(),
                       a.w() * b.x() + a.x() * b.w() + a.y() * b.z() - a.z() * b.y(),
                       a.w() * b.y() + a.y() * b.w() + a.z() * b.x() - a.x() * b.z(),
                       a.w() * b.z() + a.z() * b.w() + a.x() * b.y() - a.y() * b.x());
}
inline Quaterniond quat_conjugate(const Quaterniond &q) { return Quaterniond(q.w(), -q.x(), -q.y(), -q.z()); }
// QuaternionBase::_transformVector
inline Vector3d quat_transform(const Quaterniond &q, const Vector3d &v) {
    double u0 = q.y() * v(2) - q.z() * v(1), u1 = q.z() * v(0) - q.x() * v(2), u2 = q.x() * v(1) - q.y() * v(0);
    u0 = u0 + u0; u1 = u1 + u1; u2 = u2 + u2;
    return Vector3d(v(0) + q.w() * u0 + (q.y() * u2 - q.z() * u1), v(1) + q.w() * u1 + (q.z() * u0 - q.x() * u2),
                    v(2) + q.w() * u2 + (q.x() * u1 - q.y() * u0));
}

}  // namespace Eigen

namespace g2o {

using Eigen::Matrix3d;
using Eigen::Quaterniond;
using Eigen::Vector3d;

template <class M> class SparseBlockMatrix {};

// types/slam3d/se3quat.h as far as Converter.cc names it (no routine of this build is driven through it)
class SE3Quat {
 public:
    SE3Quat() {}
    SE3Quat(const Matrix3d &R, const Vector3d &t) : r_(R), t_(t) { r_.normalize(); }
    Eigen::Matrix4d to_homogeneous_matrix() const {
        Eigen::Matrix4d m;
        const Matrix3d R = r_.toRotationMatrix();
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) m(i, j) = i < 3 ? (j < 3 ? R(i, j) : t_(i)) : (j == 3 ? 1.0 : 0.0);
        return m;
    }
    const Quaterniond &rotation() const { return r_; }
    const Vector3d &translation() const { return t_; }

 private:
    Quaterniond r_;
    Vector3d t_ = Vector3d(0.0, 0.0, 0.0);
};

class Sim3 {
 public:
    Sim3() {}
    Sim3(const Quaterniond &r, const Vector3d &t, double s) : r_(r), t_(t), s_(s) {}
    Sim3(const Matrix3d &R, const Vector3d &t, double s) : r_(Quaterniond(R)), t_(t), s_(s) {}
    Vector3d map(const Vector3d &xyz) const {
        const Vector3d r = Eigen::quat_transform(r_, xyz);
        return Vector3d(s_ * r(0) + t_(0), s_ * r(1) + t_(1), s_ * r(2) + t_(2));
    }
    Sim3 inverse() const {
        const Quaterniond c = Eigen::quat_conjugate(r_);
        const double f = -1. / s_;
        return Sim3(c, Eigen::quat_transform(c, Vector3d(f * t_(0), f * t_(1), f * t_(2))), 1. / s_);
    }
    Sim3 operator*(const Sim3 &other) const {
        const Vector3d r = Eigen::quat_transform(r_, other.t_);
        return Sim3(Eigen::quat_product(r_, other.r_), Vector3d(s_ * r(0) + t_(0), s_ * r(1) + t_(1), s_ * r(2) + t_(2)), s_ * other.s_);
    }
    const Quaterniond &rotation() const { return r_; }
    const Vector3d &translation() const { return t_; }
    const double &scale() const { return s_; }

 private:
    Quaterniond r_;
    Vector3d t_ = Vector3d(0.0, 0.0, 0.0);
    double s_ = 1.0;
};

}  // namespace g2o
