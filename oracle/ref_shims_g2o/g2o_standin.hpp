// g2o stand-in — TEST INFRASTRUCTURE ONLY.  g2o is an un-vendored submodule of the reference (.gitmodules:4-6), so its
// src/orbslam/Optimizer.cc cannot be built as shipped.  With this header in place of <g2o/...> it compiles UNTOUCHED, from where
// it lies (oracle/Makefile `ref` -> oracle/_ref/ref_optimizer.o), and RUNS: everything the reference's code decides — which
// observations become mono / stereo edges with which information and kernel, which vertices are fixed, the sequence of
// initializeOptimization / optimize(n) calls, the chi2 re-classification with setLevel / setRobustKernel(nullptr), when
// computeError is refreshed, what is erased and written back — is the reference's.  What g2o itself would do behind those calls is
// delegated to the oracle's restatement of it:
//     SparseOptimizer::optimize(n)        -> orc_g2o_optimize (oracle/ba_solve_oracle.c: Levenberg-Marquardt over BlockSolver_6_3
//                                            with the Schur complement; only active edges get a fresh error vector)
//     Edge::computeError / chi2 /          -> orc_edge_error (oracle/ba_oracle.c arithmetic), chi2 = err' Omega err on the STORED
//       isDepthPositive                       error vector, isDepthPositive on the current estimates — as the g2o edge classes do
//     computeMarginals(spinv, v)          -> inverse of v's block of the Hpp the last buildSystem left (BlockSolver::computeMarginals
//                                            factorises Hpp, not the Schur complement)
// vertex / edge bookkeeping follows g2o: vertices by id, edges in insertion order, free pose vertices take their Hessian index in
// ascending id order, an edge with a missing vertex is refused.  So tests/cpp/pin_optimizer.cpp pins the graph walk and the
// schedules of sivo_amd/api/orbslam/OptimizerAdapter.h (+ the schedules restated inside orc_pose_optimize / orc_local_ba, and on
// the GPU leg the device solver) against the reference's own source; the numerics of g2o stay a restatement.
// The Sim3 types exist so that OptimizeEssentialGraph / OptimizeSim3 compile; their optimize() is not implemented (abort).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <vector>

#include "eigen_g2o_ext.hpp"

extern "C" {
struct OrcEdgeC {
    int32_t pose, point, stereo, pad_;
    double obs[3];
    double inv_sigma2;
};
int orc_g2o_optimize(double *poses, const uint8_t *fixed, int nP, double *points, int nX, int points_fixed, const OrcEdgeC *edges, int64_t nE,
                     const double *intr, double delta_mono, double delta_stereo, const uint8_t *level, const uint8_t *robust, int iterations,
                     double *err, double *hpp_last, const volatile uint8_t *stop_byte, int *trials);
int orc_inv6_spd(const double *H, double *out);
void orc_edge_error(const double *pose, const double *point, const OrcEdgeC *edge, const double *intr, double *err3, int *depth_positive);
}

namespace g2o {

using Eigen::Matrix3d;
using Eigen::Vector3d;
typedef Eigen::Matrix<double, 2, 1> Vector2d;

// SE3Quat(R, t): _r(Quaterniond(R)), normalizeRotation() (w >= 0, unit norm) — g2o/types/slam3d/se3quat.h
class SE3Quat {
 public:
    SE3Quat() { R_ = Matrix3d::Identity(); }
    SE3Quat(const Matrix3d &R, const Vector3d &t) : t_(t) {
        Eigen::Quaterniond q(R);
        if (q.w() < 0) q.negate();
        q.normalize();
        R_ = q.toRotationMatrix();
    }
    static SE3Quat from_pose12(const double *p) {
        SE3Quat s;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) s.R_(r, c) = p[3 * r + c];
            s.t_(r) = p[9 + r];
        }
        return s;
    }
    void to_pose12(double *p) const {
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) p[3 * r + c] = R_(r, c);
            p[9 + r] = t_(r);
        }
    }
    Eigen::Matrix4d to_homogeneous_matrix() const {
        Eigen::Matrix4d m;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) m(r, c) = R_(r, c);
            m(r, 3) = t_(r);
        }
        m(3, 3) = 1.0;
        return m;
    }
    struct Rot { Matrix3d R; Matrix3d toRotationMatrix() const { return R; } };
    Rot rotation() const { return Rot{R_}; }
    Vector3d translation() const { return t_; }

 private:
    Matrix3d R_;
    Vector3d t_;
};

// g2o::Sim3 (types/sim3/sim3.h) as far as the reference's code calls it
class Sim3 {
 public:
    Sim3() { R_ = Matrix3d::Identity(); }
    Sim3(const Matrix3d &R, const Vector3d &t, double s) : t_(t), s_(s) {
        Eigen::Quaterniond q(R);
        q.normalize();
        R_ = q.toRotationMatrix();
    }
    SE3Quat::Rot rotation() const { return SE3Quat::Rot{R_}; }
    Vector3d translation() const { return t_; }
    double scale() const { return s_; }
    Vector3d map(const Vector3d &x) const { return s_ * (R_ * x) + t_; }
    Sim3 inverse() const {
        Sim3 r;
        r.R_ = R_.transpose();
        r.s_ = 1.0 / s_;
        r.t_ = (-r.s_) * (r.R_ * t_);
        return r;
    }
    Sim3 operator*(const Sim3 &o) const {
        Sim3 r;
        r.R_ = R_ * o.R_;
        r.t_ = s_ * (R_ * o.t_) + t_;
        r.s_ = s_ * o.s_;
        return r;
    }

 private:
    Matrix3d R_;
    Vector3d t_;
    double s_ = 1.0;
};

class RobustKernel {
 public:
    virtual ~RobustKernel() {}
    void setDelta(double d) { delta_ = d; }
    double delta() const { return delta_; }

 private:
    double delta_ = 1.0;
};
class RobustKernelHuber : public RobustKernel {};

class SparseOptimizer;

class OptimizableGraph {
 public:
    class Vertex {
     public:
        virtual ~Vertex() {}
        void setId(int id) { id_ = id; }
        int id() const { return id_; }
        void setFixed(bool f) { fixed_ = f; }
        bool fixed() const { return fixed_; }
        void setMarginalized(bool m) { marginalized_ = m; }
        bool marginalized() const { return marginalized_; }
        int hessianIndex() const { return hessian_index_; }
        int hessian_index_ = -1;

     private:
        int id_ = -1;
        bool fixed_ = false, marginalized_ = false;
    };
    class Edge {
     public:
        virtual ~Edge() { delete kernel_; }
        void setVertex(size_t i, Vertex *v) {
            if (v_.size() <= i) v_.resize(i + 1, nullptr);
            v_[i] = v;
        }
        Vertex *vertex(size_t i) const { return i < v_.size() ? v_[i] : nullptr; }
        const std::vector<Vertex *> &vertices() const { return v_; }
        void setLevel(int l) { level_ = l; }
        int level() const { return level_; }
        void setRobustKernel(RobustKernel *k) { delete kernel_; kernel_ = k; }      // (g2o deletes the kernel it held)
        RobustKernel *robustKernel() const { return kernel_; }
        virtual void computeError() = 0;
        virtual double chi2() const = 0;

     protected:
        std::vector<Vertex *> v_;
        int level_ = 0;
        RobustKernel *kernel_ = nullptr;
    };
};

class VertexSE3Expmap : public OptimizableGraph::Vertex {
 public:
    void setEstimate(const SE3Quat &e) { est_ = e; }
    const SE3Quat &estimate() const { return est_; }

 private:
    SE3Quat est_;
};
class VertexSBAPointXYZ : public OptimizableGraph::Vertex {
 public:
    void setEstimate(const Vector3d &e) { est_ = e; }
    const Vector3d &estimate() const { return est_; }

 private:
    Vector3d est_;
};

// The four projection edges of types_six_dof_expmap.h behind one implementation.  vertex 0 = point, vertex 1 = pose for the
// binary edges; the only-pose edges have vertex 0 = pose and hold the point (Xw).
class ProjectionEdge : public OptimizableGraph::Edge {
 public:
    double fx = 0, fy = 0, cx = 0, cy = 0, bf = 0;
    double Xw[3] = {0, 0, 0};                    // only-pose edges: the map point, a constant
    double err[3] = {0, 0, 0};                   // what the last computeError / computeActiveErrors left
    const bool stereo, only_pose;
    ProjectionEdge(bool stereo_, bool only_pose_) : stereo(stereo_), only_pose(only_pose_) {}

    template <int N>
    void setMeasurement(const Eigen::Matrix<double, N, 1> &m) {
        static_assert(N == 2 || N == 3, "measurement");
        for (int i = 0; i < N; ++i) obs_[i] = m(i);
    }
    template <int N>
    void setInformation(const Eigen::Matrix<double, N, N> &m) { info_ = m(0, 0); }            // (the reference always sets Identity * invSigma2)
    double information00() const { return info_; }
    const double *measurement() const { return obs_; }

    VertexSE3Expmap *poseVertex() const { return dynamic_cast<VertexSE3Expmap *>(vertex(only_pose ? 0 : 1)); }
    VertexSBAPointXYZ *pointVertex() const { return only_pose ? nullptr : dynamic_cast<VertexSBAPointXYZ *>(vertex(0)); }
    void current(double pose[12], double X[3]) const {
        poseVertex()->estimate().to_pose12(pose);
        if (only_pose) { X[0] = Xw[0]; X[1] = Xw[1]; X[2] = Xw[2]; }
        else { const Vector3d &p = pointVertex()->estimate(); X[0] = p(0); X[1] = p(1); X[2] = p(2); }
    }
    OrcEdgeC record() const {
        OrcEdgeC e{};
        e.stereo = stereo ? 1 : 0;
        e.obs[0] = obs_[0]; e.obs[1] = obs_[1]; e.obs[2] = stereo ? obs_[2] : 0.0;
        e.inv_sigma2 = info_;
        return e;
    }
    void computeError() override {
        double pose[12], X[3];
        current(pose, X);
        const OrcEdgeC e = record();
        const double intr[5] = {fx, fy, cx, cy, bf};
        orc_edge_error(pose, X, &e, intr, err, nullptr);
    }
    double chi2() const override { return (err[0] * err[0] + err[1] * err[1] + err[2] * err[2]) * info_; }
    bool isDepthPositive() const {
        double pose[12], X[3], tmp[3];
        current(pose, X);
        const OrcEdgeC e = record();
        const double intr[5] = {fx, fy, cx, cy, bf};
        int ok = 0;
        orc_edge_error(pose, X, &e, intr, tmp, &ok);
        return ok != 0;
    }

 private:
    double obs_[3] = {0, 0, 0};
    double info_ = 1.0;
};
class EdgeSE3ProjectXYZ : public ProjectionEdge { public: EdgeSE3ProjectXYZ() : ProjectionEdge(false, false) {} };
class EdgeStereoSE3ProjectXYZ : public ProjectionEdge { public: EdgeStereoSE3ProjectXYZ() : ProjectionEdge(true, false) {} };
class EdgeSE3ProjectXYZOnlyPose : public ProjectionEdge { public: EdgeSE3ProjectXYZOnlyPose() : ProjectionEdge(false, true) {} };
class EdgeStereoSE3ProjectXYZOnlyPose : public ProjectionEdge { public: EdgeStereoSE3ProjectXYZOnlyPose() : ProjectionEdge(true, true) {} };

// ---- Sim3 types: compile-only
class VertexSim3Expmap : public OptimizableGraph::Vertex {
 public:
    void setEstimate(const Sim3 &e) { est_ = e; }
    const Sim3 &estimate() const { return est_; }
    bool _fix_scale = false;
    double _principle_point1[2] = {0, 0}, _principle_point2[2] = {0, 0}, _focal_length1[2] = {0, 0}, _focal_length2[2] = {0, 0};

 private:
    Sim3 est_;
};
class Sim3Edge : public OptimizableGraph::Edge {
 public:
    void setMeasurement(const Sim3 &) {}
    template <int N> void setMeasurement(const Eigen::Matrix<double, N, 1> &) {}
    template <int N> void setInformation(const Eigen::Matrix<double, N, N> &) {}
    Eigen::Matrix7d &information() { return info7_; }
    void computeError() override {}
    double chi2() const override { return 0.0; }

 private:
    Eigen::Matrix7d info7_;
};
class EdgeSim3 : public Sim3Edge {};
class EdgeSim3ProjectXYZ : public Sim3Edge {};
class EdgeInverseSim3ProjectXYZ : public Sim3Edge {};

// ---- solver scaffolding: types only (the solve is the oracle's)
template <class M> class LinearSolver { public: virtual ~LinearSolver() {} };
template <class M> class LinearSolverCholmod : public LinearSolver<M> {};
template <class M> class LinearSolverEigen : public LinearSolver<M> {};
template <class M> class LinearSolverDense : public LinearSolver<M> {};
template <int P, int L>
class BlockSolverPL {
 public:
    typedef Eigen::MatrixXd PoseMatrixType;
    typedef LinearSolver<PoseMatrixType> LinearSolverType;
    explicit BlockSolverPL(LinearSolverType *ls) : ls_(ls) {}
    ~BlockSolverPL() { delete ls_; }
    static constexpr int pose_dim = P, landmark_dim = L;

 private:
    LinearSolverType *ls_;
};
typedef BlockSolverPL<6, 3> BlockSolver_6_3;
typedef BlockSolverPL<7, 3> BlockSolver_7_3;
typedef BlockSolverPL<-1, -1> BlockSolverX;
class OptimizationAlgorithm { public: virtual ~OptimizationAlgorithm() {} int pose_dim = 6; };
class OptimizationAlgorithmLevenberg : public OptimizationAlgorithm {
 public:
    template <int P, int L>
    explicit OptimizationAlgorithmLevenberg(BlockSolverPL<P, L> *s) : holder_(s, [](void *p) { delete static_cast<BlockSolverPL<P, L> *>(p); }) { pose_dim = P; }
    void setUserLambdaInit(double) {}

 private:
    std::shared_ptr<void> holder_;
};

template <class M>
class SparseBlockMatrix {
 public:
    M *block(int r, int c) {
        const auto it = blocks_.find(std::make_pair(r, c));
        return it == blocks_.end() ? nullptr : &it->second;
    }
    std::map<std::pair<int, int>, M> blocks_;
};

class SparseOptimizer {
 public:
    ~SparseOptimizer() {
        for (auto *e : edges_) delete e;
        for (auto &v : vertices_) delete v.second;
        delete algorithm_;
    }
    void setAlgorithm(OptimizationAlgorithm *a) { delete algorithm_; algorithm_ = a; }
    void setForceStopFlag(bool *flag) { stop_ = flag; }
    void setVerbose(bool) {}
    bool addVertex(OptimizableGraph::Vertex *v) {
        if (vertices_.count(v->id())) return false;
        vertices_[v->id()] = v;
        inserted_.push_back(v);
        return true;
    }
    bool removeVertex(OptimizableGraph::Vertex *v) {
        for (size_t i = 0; i < edges_.size();) {
            bool uses = false;
            for (auto *ev : edges_[i]->vertices()) uses = uses || ev == v;
            if (uses) { delete edges_[i]; edges_.erase(edges_.begin() + (long)i); } else ++i;
        }
        vertices_.erase(v->id());
        for (size_t i = 0; i < inserted_.size(); ++i)
            if (inserted_[i] == v) { inserted_.erase(inserted_.begin() + (long)i); break; }
        delete v;
        return true;
    }
    bool addEdge(OptimizableGraph::Edge *e) {
        for (auto *v : e->vertices())
            if (!v) return false;                   // HyperGraph::addEdge refuses an edge with a missing vertex
        edges_.push_back(e);
        return true;
    }
    bool removeEdge(OptimizableGraph::Edge *e) {
        for (size_t i = 0; i < edges_.size(); ++i)
            if (edges_[i] == e) { delete e; edges_.erase(edges_.begin() + (long)i); return true; }
        return false;
    }
    OptimizableGraph::Vertex *vertex(int id) {
        const auto it = vertices_.find(id);
        return it == vertices_.end() ? nullptr : it->second;
    }
    const std::vector<OptimizableGraph::Edge *> &edges() const { return edges_; }
    const std::vector<OptimizableGraph::Vertex *> &verticesInInsertionOrder() const { return inserted_; }
    // The recording mode (oracle/ref_bawindow_driver.cpp): a hook that is handed the graph at initializeOptimization, before anything is
    // solved; it may throw to leave the optimisation there.  Empty in every other program.
    static std::function<void(const SparseOptimizer &)> &recordHook() { static std::function<void(const SparseOptimizer &)> h; return h; }

    // active set = the edges of that level; free pose vertices get their Hessian index in ascending id order
    bool initializeOptimization(int level = 0) {
        active_level_ = level;
        if (recordHook()) recordHook()(*this);
        return true;
    }
    int optimize(int iterations) {
        if (algorithm_ && algorithm_->pose_dim != 6) { std::fprintf(stderr, "g2o stand-in: Sim3 optimisation is not implemented\n"); std::abort(); }
        // vertices -> arrays (ascending id: the order of g2o's active vertex list)
        std::vector<VertexSE3Expmap *> pv;
        std::vector<VertexSBAPointXYZ *> xv;
        std::map<const OptimizableGraph::Vertex *, int> index;
        for (auto &kv : vertices_) {
            if (auto *p = dynamic_cast<VertexSE3Expmap *>(kv.second)) { index[p] = (int)pv.size(); pv.push_back(p); }
            else if (auto *x = dynamic_cast<VertexSBAPointXYZ *>(kv.second)) { index[x] = (int)xv.size(); xv.push_back(x); }
        }
        std::vector<double> poses(12 * pv.size());
        std::vector<uint8_t> fixed(pv.size());
        int nfree = 0;
        for (size_t i = 0; i < pv.size(); ++i) {
            pv[i]->estimate().to_pose12(poses.data() + 12 * i);
            fixed[i] = pv[i]->fixed() ? 1 : 0;
            pv[i]->hessian_index_ = pv[i]->fixed() ? -1 : nfree++;
        }
        std::vector<ProjectionEdge *> pe;
        for (auto *e : edges_)
            if (auto *q = dynamic_cast<ProjectionEdge *>(e)) pe.push_back(q);
        bool only_pose = !pe.empty() && pe[0]->only_pose;
        std::vector<double> points;
        if (only_pose) points.resize(3 * pe.size());
        else {
            points.resize(3 * xv.size());
            for (size_t i = 0; i < xv.size(); ++i)
                for (int r = 0; r < 3; ++r) points[3 * i + r] = xv[i]->estimate()(r);
        }
        std::vector<OrcEdgeC> rec(pe.size());
        std::vector<uint8_t> level(pe.size()), robust(pe.size());
        std::vector<double> err(3 * pe.size());
        double intr[5] = {0, 0, 0, 0, 0}, delta_mono = 0, delta_stereo = 0;
        for (size_t i = 0; i < pe.size(); ++i) {
            ProjectionEdge *e = pe[i];
            if (e->only_pose != only_pose) { std::fprintf(stderr, "g2o stand-in: mixed edge kinds\n"); std::abort(); }
            rec[i] = e->record();
            rec[i].pose = index.at(e->poseVertex());
            if (only_pose) { rec[i].point = (int)i; for (int r = 0; r < 3; ++r) points[3 * i + r] = e->Xw[r]; }
            else rec[i].point = index.at(e->pointVertex());
            level[i] = e->level() == active_level_ ? 0 : 1;
            robust[i] = e->robustKernel() ? 1 : 0;
            if (e->robustKernel()) (e->stereo ? delta_stereo : delta_mono) = e->robustKernel()->delta();
            for (int r = 0; r < 3; ++r) err[3 * i + r] = e->err[r];
            if (i == 0) { intr[0] = e->fx; intr[1] = e->fy; intr[2] = e->cx; intr[3] = e->cy; }
            if (e->stereo) intr[4] = e->bf;
        }
        hpp_last_.assign(36 * (size_t)(nfree ? nfree : 1), 0.0);
        const int n = orc_g2o_optimize(poses.data(), fixed.data(), (int)pv.size(), points.data(), only_pose ? (int)pe.size() : (int)xv.size(), only_pose ? 1 : 0,
                                       rec.data(), (int64_t)rec.size(), intr, delta_mono, delta_stereo, level.data(), robust.data(), iterations, err.data(),
                                       hpp_last_.data(), reinterpret_cast<const volatile uint8_t *>(stop_), nullptr);
        for (size_t i = 0; i < pv.size(); ++i)
            if (!pv[i]->fixed()) pv[i]->setEstimate(SE3Quat::from_pose12(poses.data() + 12 * i));
        if (!only_pose)
            for (size_t i = 0; i < xv.size(); ++i) xv[i]->setEstimate(Vector3d(points[3 * i], points[3 * i + 1], points[3 * i + 2]));
        for (size_t i = 0; i < pe.size(); ++i)
            for (int r = 0; r < 3; ++r) pe[i]->err[r] = err[3 * i + r];
        return n;
    }
    // BlockSolver::computeMarginals: the block pair (hessianIndex(v), hessianIndex(v)) of inv(Hpp), Hpp of the last buildSystem
    bool computeMarginals(SparseBlockMatrix<Eigen::MatrixXd> &spinv, const OptimizableGraph::Vertex *v) {
        const int h = v->hessianIndex();
        if (h < 0 || hpp_last_.size() < 36 * (size_t)(h + 1)) return false;
        double inv[36];
        if (!orc_inv6_spd(hpp_last_.data() + 36 * (size_t)h, inv)) return false;
        Eigen::MatrixXd m(6, 6);
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) m(r, c) = inv[6 * r + c];
        spinv.blocks_[std::make_pair(h, h)] = m;
        return true;
    }

 private:
    std::map<int, OptimizableGraph::Vertex *> vertices_;
    std::vector<OptimizableGraph::Edge *> edges_;
    std::vector<OptimizableGraph::Vertex *> inserted_;       // the vertices in the order addVertex took them
    OptimizationAlgorithm *algorithm_ = nullptr;
    bool *stop_ = nullptr;
    int active_level_ = 0;
    std::vector<double> hpp_last_;
};



}  // namespace g2o
