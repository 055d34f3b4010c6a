// select.hip — SIVO's information-theoretic map-point selection gate, batched over the semantic
// keypoints of a frame.  Stands behind
//   SIVO::computeStereoJacobianPose / computeStereoCovariance / computeStereoMutualInformation
//   (reference src/sivo_helpers/sivo_helpers.cpp:64-88, 160-180, 201-219)
// as they are applied in
//   Tracking::CreateNewKeyFrame (reference src/orbslam/Tracking.cc:934-1023): entropy lookup at the truncated keypoint
//     position in the entropy map the SegNet path left in HBM, depth > 0, accept iff MI - entropy > ThEntropyReduction
//     (sivo_entropy_gate);
//   LocalMapping::CheckSemantics (reference src/orbslam/LocalMapping.cc:474-538, compute_information = true): also a
//     static class (<= TERRAIN) and confidence >= ThConfidence, and the point is rejected only when
//     MI - entropy < ThEntropyReduction, i.e. it passes at equality (sivo_check_semantics).
// One thread per keypoint, fp64, determinants as Eigen takes them (3x3 cofactors, 6x6 / 9x9 partial-
// pivot LU); a few thousand independent 9x9 factorizations: latency bound, microseconds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "gate_math.hpp"
#include "solver_host.hpp"

namespace sivo {

struct GateArgs {
    const SivoKeyPoint *kps;
    const float *depth;
    const double *xyz;
    const double *entropy;
    int rows, cols, n;
    double Sx[36];
    double fx, fy, bl, th;
    float level_sigma2[16];
    int nlevels;                       // a key whose octave is outside [0, nlevels) fails the gate: level_sigma2[] is never indexed with it
    double *mi, *reduction;
    uint8_t *accept;
    // CheckSemantics form (classes != nullptr): accept[] receives the detected class, or VOID (255)
    const double *confidence;
    const uint8_t *classes;
    double th_conf;
};

__global__ void entropy_gate_kernel(GateArgs g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n) return;
    double m = 0.0, red = 0.0;
    uint8_t acc = 0;
    const SivoKeyPoint kp = g.kps[i];
    const int col = (int)kp.x, row = (int)kp.y;
    bool ok = g.depth[i] > 0 && row >= 0 && row < g.rows && col >= 0 && col < g.cols && kp.octave >= 0 && kp.octave < g.nlevels;
    int cls = 255;
    if (g.classes) {
        acc = 255;                                                   // Classes::VOID
        if (ok) {
            cls = g.classes[(int64_t)row * g.cols + col];
            ok = cls <= 8 && g.confidence[(int64_t)row * g.cols + col] >= g.th_conf;     // <= Classes::TERRAIN, >= mThConfidence
        }
    }
    if (ok) {
        const double X = g.xyz[3 * i], Y = g.xyz[3 * i + 1], Z = g.xyz[3 * i + 2];
        m = gate_mutual_information(g.Sx, g.fx, g.fy, g.bl, X, Y, Z, (double)g.level_sigma2[kp.octave]);
        red = m - g.entropy[(int64_t)row * g.cols + col];
        if (g.classes) acc = red < g.th ? 255 : (uint8_t)cls;         // LocalMapping.cc:529-532: rejected only below the threshold
        else acc = red > g.th;
    }
    if (g.mi) g.mi[i] = m;
    if (g.reduction) g.reduction[i] = red;
    if (g.accept) g.accept[i] = acc;
}

}  // namespace sivo

using namespace sivo;

// Host-array entry points: every key's octave is looked at before anything is staged or launched, so that a bad one
// leaves the outputs as they were (the device-resident forms cannot look: there the kernel fails such a key).
static void require_octaves(const SivoKeyPoint *kps, int n, int nlevels) {
    if (nlevels < 1 || nlevels > 16) throw std::invalid_argument("bad sizes (nlevels <= 16)");
    for (int i = 0; i < n; ++i)
        if (kps[i].octave < 0 || kps[i].octave >= nlevels) throw std::invalid_argument("keypoint octave outside [0, nlevels)");
}

extern "C" int sivo_entropy_gate_dev(int n, const SivoKeyPoint *d_kps, const float *d_depth, const double *d_xyz,
                                     const double *d_entropy, int rows, int cols, const double state_cov[36], double fx,
                                     double fy, double bl, const float *level_sigma2, int nlevels, double th,
                                     double *d_mi, double *d_reduction, uint8_t *d_accept, void *stream) {
    return guarded([&] {
        if (n < 0 || nlevels < 1 || nlevels > 16) throw std::invalid_argument("bad sizes (nlevels <= 16)");
        if (n == 0) return SIVO_OK;
        if (!d_kps || !d_depth || !d_xyz || !d_entropy || !state_cov || !level_sigma2) throw std::invalid_argument("null argument");
        GateArgs g{};
        g.kps = d_kps; g.depth = d_depth; g.xyz = d_xyz; g.entropy = d_entropy; g.rows = rows; g.cols = cols; g.n = n;
        for (int i = 0; i < 36; ++i) g.Sx[i] = state_cov[i];
        g.fx = fx; g.fy = fy; g.bl = bl; g.th = th;
        for (int i = 0; i < nlevels; ++i) g.level_sigma2[i] = level_sigma2[i];
        g.nlevels = nlevels;
        g.mi = d_mi; g.reduction = d_reduction; g.accept = d_accept;
        hipLaunchKernelGGL(entropy_gate_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, g);
        SIVO_HIP(hipGetLastError());
        return SIVO_OK;
    });
}

// Host keypoints against the entropy map the network left in HBM (the per-frame form: the keys come out of the semantic filter on
// the host, the 2.9 MB f64 map never has to leave the device for this).  The key arrays are staged into a pinned buffer of the
// calling thread which the kernel reads directly, and the three outputs are written straight into pinned memory: one launch, one
// synchronisation, no allocation once the buffers fit.  The caller has synchronised with whatever produced d_entropy (the frame
// has: it reads the class map back before it filters the keys).
extern "C" int sivo_entropy_gate_map_dev(int n, const SivoKeyPoint *kps, const float *depth, const double *xyz,
                                         const double *d_entropy, int rows, int cols, const double state_cov[36], double fx,
                                         double fy, double bl, const float *level_sigma2, int nlevels, double th, double *mi,
                                         double *reduction, uint8_t *accept) {
    return guarded([&] {
        if (n < 0) throw std::invalid_argument("negative size");
        if (n == 0) return SIVO_OK;
        if (!kps || !depth || !xyz || !d_entropy) throw std::invalid_argument("null argument");
        require_octaves(kps, n, nlevels);
        require_device();
        // (a dozen workgroups that a host thread waits for: a high-priority stream, ahead of whatever else the device is running)
        static thread_local SolverCtx c(true, 256 << 10, 0, 0);
        c.bind();
        const size_t N = (size_t)n;
        const SivoKeyPoint *h_kps; const float *h_depth; const double *h_xyz; double *h_mi, *h_red; uint8_t *h_acc;
        Layout L;                             // (all of it in the pinned buffer, where the kernel reads and writes it)
        L.copy(h_xyz, xyz, N * 24); L.copy(h_kps, kps, N * sizeof(SivoKeyPoint)); L.copy(h_depth, depth, N * 4);
        L.take(h_mi, N * 8); L.take(h_red, N * 8); L.take(h_acc, N);
        char *h = c.in.reserve(L.bytes());
        L.place(h, h);
        const int rc = sivo_entropy_gate_dev(n, h_kps, h_depth, h_xyz, d_entropy, rows, cols, state_cov, fx, fy, bl, level_sigma2, nlevels, th,
                                             h_mi, h_red, h_acc, c.stream);
        if (rc) return rc;
        SIVO_HIP(hipStreamSynchronize(c.stream));
        if (mi) std::memcpy(mi, h_mi, N * 8);
        if (reduction) std::memcpy(reduction, h_red, N * 8);
        if (accept) std::memcpy(accept, h_acc, N);
        return SIVO_OK;
    });
}

extern "C" int sivo_check_semantics_dev(int n, const SivoKeyPoint *d_kps, const float *d_depth, const double *d_xyz,
                                        const double *d_entropy, const double *d_confidence, const uint8_t *d_classes, int rows,
                                        int cols, const double state_cov[36], double fx, double fy, double bl,
                                        const float *level_sigma2, int nlevels, double th_entropy, double th_confidence,
                                        double *d_mi, double *d_reduction, uint8_t *d_detected_class, void *stream) {
    return guarded([&] {
        if (n < 0 || nlevels < 1 || nlevels > 16) throw std::invalid_argument("bad sizes (nlevels <= 16)");
        if (n == 0) return SIVO_OK;
        if (!d_kps || !d_depth || !d_xyz || !d_entropy || !d_confidence || !d_classes || !state_cov || !level_sigma2 || !d_detected_class)
            throw std::invalid_argument("null argument");
        GateArgs g{};
        g.kps = d_kps; g.depth = d_depth; g.xyz = d_xyz; g.entropy = d_entropy; g.rows = rows; g.cols = cols; g.n = n;
        for (int i = 0; i < 36; ++i) g.Sx[i] = state_cov[i];
        g.fx = fx; g.fy = fy; g.bl = bl; g.th = th_entropy;
        for (int i = 0; i < nlevels; ++i) g.level_sigma2[i] = level_sigma2[i];
        g.nlevels = nlevels;
        g.mi = d_mi; g.reduction = d_reduction; g.accept = d_detected_class;
        g.confidence = d_confidence; g.classes = d_classes; g.th_conf = th_confidence;
        hipLaunchKernelGGL(entropy_gate_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, g);
        SIVO_HIP(hipGetLastError());
        return SIVO_OK;
    });
}

extern "C" int sivo_check_semantics(int n, const SivoKeyPoint *kps, const float *depth, const double *xyz, const double *entropy,
                                    const double *confidence, const uint8_t *classes, int rows, int cols, const double state_cov[36],
                                    double fx, double fy, double bl, const float *level_sigma2, int nlevels, double th_entropy,
                                    double th_confidence, double *mi, double *reduction, uint8_t *detected_class) {
    return guarded([&] {
        if (n < 0) throw std::invalid_argument("negative size");
        if (n == 0) return SIVO_OK;
        if (!kps || !depth || !xyz || !entropy || !confidence || !classes || !detected_class) throw std::invalid_argument("null argument");
        require_octaves(kps, n, nlevels);
        require_device();
        CallBuf dk, dd, dx, de, dc, dl, dm, dr, da;
        const size_t px = (size_t)rows * cols;
        dk.up(kps, (size_t)n * sizeof(SivoKeyPoint)); dd.up(depth, (size_t)n * 4); dx.up(xyz, (size_t)n * 24);
        de.up(entropy, px * 8); dc.up(confidence, px * 8); dl.up(classes, px);
        dm.up(nullptr, (size_t)n * 8); dr.up(nullptr, (size_t)n * 8); da.up(nullptr, (size_t)n);
        const int rc = sivo_check_semantics_dev(n, (const SivoKeyPoint *)dk.p, (const float *)dd.p, (const double *)dx.p, (const double *)de.p,
                                                (const double *)dc.p, (const uint8_t *)dl.p, rows, cols, state_cov, fx, fy, bl, level_sigma2,
                                                nlevels, th_entropy, th_confidence, (double *)dm.p, (double *)dr.p, (uint8_t *)da.p, nullptr);
        if (rc) return rc;
        if (mi) SIVO_HIP(hipMemcpy(mi, dm.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (reduction) SIVO_HIP(hipMemcpy(reduction, dr.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        SIVO_HIP(hipMemcpy(detected_class, da.p, (size_t)n, hipMemcpyDeviceToHost));
        return SIVO_OK;
    });
}

extern "C" int sivo_entropy_gate(int n, const SivoKeyPoint *kps, const float *depth, const double *xyz,
                                 const double *entropy, int rows, int cols, const double state_cov[36], double fx,
                                 double fy, double bl, const float *level_sigma2, int nlevels, double th, double *mi,
                                 double *reduction, uint8_t *accept) {
    return guarded([&] {
        if (n < 0) throw std::invalid_argument("negative size");
        if (n == 0) return SIVO_OK;
        if (!kps || !depth || !xyz || !entropy) throw std::invalid_argument("null argument");
        require_octaves(kps, n, nlevels);
        require_device();
        CallBuf dk, dd, dx, de, dm, dr, da;
        dk.up(kps, (size_t)n * sizeof(SivoKeyPoint)); dd.up(depth, (size_t)n * 4); dx.up(xyz, (size_t)n * 24);
        de.up(entropy, (size_t)rows * cols * 8);
        dm.up(nullptr, (size_t)n * 8); dr.up(nullptr, (size_t)n * 8); da.up(nullptr, (size_t)n);
        const int rc = sivo_entropy_gate_dev(n, (const SivoKeyPoint *)dk.p, (const float *)dd.p, (const double *)dx.p,
                                             (const double *)de.p, rows, cols, state_cov, fx, fy, bl, level_sigma2, nlevels, th,
                                             (double *)dm.p, (double *)dr.p, (uint8_t *)da.p, nullptr);
        if (rc) return rc;
        if (mi) SIVO_HIP(hipMemcpy(mi, dm.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (reduction) SIVO_HIP(hipMemcpy(reduction, dr.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        if (accept) SIVO_HIP(hipMemcpy(accept, da.p, (size_t)n, hipMemcpyDeviceToHost));
        return SIVO_OK;
    });
}
