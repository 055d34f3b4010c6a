// loopcorrect.hip — the two map corrections of the loop closer on arrays: LoopClosing::CorrectLoop's pose propagation and point correction
// (reference src/orbslam/LoopClosing.cc:436-526, sivo_loop_correct) and the map update behind the global bundle adjustment
// (LoopClosing.cc:694-753, sivo_gba_propagate).  The arithmetic is loopcorrect_math.hpp, shared with the host programs of the tests.
//
// sivo_loop_correct: three kernels on one stream.
//   loop_keyframe_kernel   one thread per corrected keyframe: its two Sim3, the inverse of the corrected one, the new pose and centre.
//   loop_owner_kernel      one thread per slot: the keyframe of the slot by bisection of slot_off, then an integer atomicMax of
//                          n_kf - keyframe into the point's zeroed word — the first keyframe of the order wins whatever the schedule,
//                          a point that sits twice in one keyframe writes the same value twice.
//   loop_point_kernel      one thread per point.  The normal is a running float sum in observation order and the two Sim3 maps are a
//                          few dozen dependent double operations: a wavefront per point would leave 63 lanes idle behind lane 0 (as
//                          mappoint.hip's last phase does, which has the descriptor medians to share); tens of thousands of points
//                          give the machine its parallelism.  The camera centres are gathered through obs_kf either way.
// sivo_gba_propagate: two kernels.
//   gba_keyframe_kernel    one thread per keyframe walks up its parents to the nearest one inside the BA (the host's argument check,
//                          which visits every keyframe once to rule out cycles, also leaves which keyframes hang below an origin)
//                          and recomputes its chain of poses outside the BA downward; no thread waits for another.
//   gba_point_kernel       one thread per point.
//
// Host side: the argument checks, one staged upload and one download per call on the staging helpers of solver_host.hpp; nothing is
// allocated once the buffers fit, nothing stays resident.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <stdexcept>
#include <vector>

#include "common.hpp"
#include "solver_host.hpp"

#pragma clang fp contract(off)

#include "loopcorrect_math.hpp"

namespace sivo {

constexpr int LC_THREADS = 256;

struct LcArgs {
    SivoLoopCorrect p;             // device pointers, inputs and outputs
    double *cor_inv;               // 8 n_kf: the inverse of CorrectedSim3
    int32_t *owner_code;           // n_points, zeroed: n_kf - (the first keyframe that holds the point), 0 = none
    float *geom;                   // 5 n_points: max, min, normal[3]
    int64_t n_slots;
};

__global__ __launch_bounds__(LC_THREADS) void loop_keyframe_kernel(LcArgs a) {
    const int i = blockIdx.x * LC_THREADS + (int)threadIdx.x;
    if (i >= a.p.n_kf) return;
    lc_keyframe(a.p, i, a.p.noncorrected_siw + 8 * (int64_t)i, a.p.corrected_siw + 8 * (int64_t)i, a.cor_inv + 8 * (int64_t)i,
                a.p.tiw_out + 16 * (int64_t)i, a.p.ow_out + 3 * (int64_t)i);
}

__global__ __launch_bounds__(LC_THREADS) void loop_owner_kernel(LcArgs a) {
    const int64_t s = (int64_t)blockIdx.x * LC_THREADS + threadIdx.x;
    if (s >= a.n_slots) return;
    const int32_t p = a.p.slot_point[s];
    if (p < 0) return;                                                  // (LoopClosing.cc:489)
    if (a.p.skip[p]) return;                                            // (:491-494)
    int lo = 0, hi = a.p.n_kf - 1;                                      // the last keyframe whose slots begin at or before s
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.p.slot_off[mid] <= s) lo = mid;
        else hi = mid - 1;
    }
    atomicMax(&a.owner_code[p], a.p.n_kf - lo);
}

__global__ __launch_bounds__(LC_THREADS) void loop_point_kernel(LcArgs a) {
    const int p = blockIdx.x * LC_THREADS + (int)threadIdx.x;
    if (p >= a.p.n_points) return;
    const int32_t code = a.owner_code[p];
    if (code == 0) {
        a.p.corrected_by[p] = -1;
        return;
    }
    const int32_t owner = a.p.n_kf - code;
    a.p.corrected_by[p] = owner;
    a.p.flags[p] = lc_point(a.p, a.p.noncorrected_siw, a.cor_inv, a.p.ow_out, owner, p, a.p.pos_out + 3 * (int64_t)p, a.geom + 5 * (int64_t)p);
}

struct GbaArgs {
    SivoGbaPropagate p;            // device pointers
    const int32_t *parent;         // n_kf
    const uint8_t *kf_flags;       // n_kf: LC_KF_ORIGIN | LC_KF_REACHED
    float *twc_after;              // 16 n_kf: GetPoseInverse() after the walk
    uint8_t *in_gba_after;         // n_kf
};

__global__ __launch_bounds__(LC_THREADS) void gba_keyframe_kernel(GbaArgs a) {
    const int k = blockIdx.x * LC_THREADS + (int)threadIdx.x;
    if (k >= a.p.n_kf) return;
    float G[16], Twc[16];
    uint8_t in_after;
    const bool reached = lc_tree_keyframe(a.p, a.parent, a.kf_flags, k, G, Twc, &in_after);
    a.p.kf_reached[k] = reached;
    a.in_gba_after[k] = in_after;
    for (int i = 0; i < 16; ++i) {
        a.p.tcw_out[16 * (int64_t)k + i] = lc_canon(G[i]);
        a.twc_after[16 * (int64_t)k + i] = Twc[i];
    }
    for (int i = 0; i < 3; ++i) a.p.ow_out[3 * (int64_t)k + i] = lc_canon(Twc[4 * i + 3]);
}

__global__ __launch_bounds__(LC_THREADS) void gba_point_kernel(GbaArgs a) {
    const int p = blockIdx.x * LC_THREADS + (int)threadIdx.x;
    if (p >= a.p.n_points) return;
    a.p.point_status[p] = lc_gba_point(a.p, a.p.kf_reached, a.twc_after, a.in_gba_after, p, a.p.pos_out + 3 * (int64_t)p);
}

static SolverCtx &lc_ctx() {
    static thread_local SolverCtx c(false, 4 << 20, 0, 4 << 20);
    c.bind();
    return c;
}

}  // namespace sivo

using namespace sivo;

extern "C" int sivo_loop_correct(const SivoLoopCorrect *problem) {
    return guarded([&] {
        if (const char *e = lc_check_loop_correct(problem)) throw std::invalid_argument(std::string("sivo_loop_correct: ") + e);
        const SivoLoopCorrect &h = *problem;
        require_device();
        SolverCtx &c = lc_ctx();
        const size_t K = (size_t)h.n_kf, A = (size_t)h.n_all, P = (size_t)h.n_points, ns = (size_t)h.slot_off[K];
        const size_t no = P ? (size_t)h.obs_off[P] : 0;
        LcArgs a;
        a.p = h;
        a.n_slots = (int64_t)ns;
        Layout L;
        L.copy(a.p.tiw, h.tiw, 64 * K); L.copy(a.p.twc_cur, h.twc_cur, 64); L.copy(a.p.scw, h.scw, 64); L.copy(a.p.ow, h.ow, 12 * A);
        L.copy(a.p.slot_off, h.slot_off, 8 * (K + 1)); L.copy(a.p.slot_point, h.slot_point, 4 * ns);
        L.copy(a.p.pos, h.pos, 12 * P); L.copy(a.p.skip, h.skip, P); L.copy(a.p.obs_off, h.obs_off, P ? 8 * (P + 1) : 0);
        L.copy(a.p.obs_kf, h.obs_kf, 4 * no); L.copy(a.p.ref_kf, h.ref_kf, 4 * P);
        L.copy(a.p.level_scale, h.level_scale, 4 * P); L.copy(a.p.last_scale, h.last_scale, 4 * P);
        L.zero(a.owner_code, 4 * P);
        L.take(a.p.noncorrected_siw, 64 * K); L.take(a.p.corrected_siw, 64 * K); L.take(a.p.tiw_out, 64 * K); L.take(a.p.ow_out, 12 * K);
        L.take(a.p.corrected_by, 4 * P); L.take(a.p.pos_out, 12 * P); L.take(a.geom, 20 * P); L.take(a.p.flags, P);
        L.take(a.cor_inv, 64 * K);                                      // scratch behind the results
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        L.send(c.stream);
        hipLaunchKernelGGL(loop_keyframe_kernel, dim3((unsigned)cdiv(h.n_kf, LC_THREADS)), dim3(LC_THREADS), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        if (ns && P) {
            hipLaunchKernelGGL(loop_owner_kernel, dim3((unsigned)cdiv64((int64_t)ns, LC_THREADS)), dim3(LC_THREADS), 0, c.stream, a);
            SIVO_HIP(hipGetLastError());
        }
        if (P) {
            hipLaunchKernelGGL(loop_point_kernel, dim3((unsigned)cdiv(h.n_points, LC_THREADS)), dim3(LC_THREADS), 0, c.stream, a);
            SIVO_HIP(hipGetLastError());
        }
        SIVO_HIP(hipMemcpyAsync(L.host(a.p.noncorrected_siw), a.p.noncorrected_siw, L.results(), hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        std::memcpy(h.noncorrected_siw, L.host(a.p.noncorrected_siw), 64 * K);
        std::memcpy(h.corrected_siw, L.host(a.p.corrected_siw), 64 * K);
        std::memcpy(h.tiw_out, L.host(a.p.tiw_out), 64 * K);
        std::memcpy(h.ow_out, L.host(a.p.ow_out), 12 * K);
        const int32_t *by = L.host(a.p.corrected_by);
        const float *hp = L.host(a.p.pos_out), *hg = L.host(a.geom);
        const uint8_t *hf = L.host(a.p.flags);
        for (size_t p = 0; p < P; ++p) {
            h.corrected_by[p] = by[p];
            if (by[p] < 0) continue;                                    // untouched: nothing else of the point is written
            std::memcpy(h.pos_out + 3 * p, hp + 3 * p, 12);
            h.flags[p] = hf[p];
            if (hf[p] & SIVO_MP_NO_OBSERVATION) continue;
            h.max_dist[p] = hg[5 * p]; h.min_dist[p] = hg[5 * p + 1];
            std::memcpy(h.normal + 3 * p, hg + 5 * p + 2, 12);
        }
        return SIVO_OK;
    });
}

extern "C" int sivo_gba_propagate(const SivoGbaPropagate *problem) {
    return guarded([&] {
        static thread_local std::vector<int32_t> parent;
        static thread_local std::vector<uint8_t> kf_flags;
        if (problem && problem->n_kf > 0 && problem->n_kf <= (1 << 24)) { parent.resize((size_t)problem->n_kf); kf_flags.resize((size_t)problem->n_kf); }
        if (const char *e = lc_check_gba_propagate(problem, parent.data(), kf_flags.data())) throw std::invalid_argument(std::string("sivo_gba_propagate: ") + e);
        const SivoGbaPropagate &h = *problem;
        if (h.n_kf == 0 && h.n_points == 0) return SIVO_OK;
        require_device();
        SolverCtx &c = lc_ctx();
        const size_t K = (size_t)h.n_kf, P = (size_t)h.n_points, nc = K ? (size_t)h.child_off[K] : 0;
        (void)nc;                                                       // the children reach the device as `parent`
        GbaArgs a;
        a.p = h;
        Layout L;
        const float *d_tcw_gba, *d_tcw_bef;
        const uint8_t *d_in_gba;
        L.copy(a.parent, parent.data(), 4 * K); L.copy(a.kf_flags, kf_flags.data(), K);
        L.copy(a.p.tcw, h.tcw, 64 * K); L.copy(d_tcw_gba, h.tcw_gba, 64 * K); L.copy(d_in_gba, h.in_gba, K); L.copy(d_tcw_bef, h.tcw_bef, 64 * K);
        L.copy(a.p.pos, h.pos, 12 * P); L.copy(a.p.pos_gba, h.pos_gba, 12 * P); L.copy(a.p.point_in_gba, h.point_in_gba, P);
        L.copy(a.p.point_bad, h.point_bad, P); L.copy(a.p.ref_kf, h.ref_kf, 4 * P);
        L.take(a.p.tcw_out, 64 * K); L.take(a.p.ow_out, 12 * K); L.take(a.p.kf_reached, K); L.take(a.in_gba_after, K);
        L.take(a.p.pos_out, 12 * P); L.take(a.p.point_status, P);
        L.take(a.twc_after, 64 * K);                                    // scratch behind the results
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        a.p.tcw_gba = const_cast<float *>(d_tcw_gba); a.p.tcw_bef = const_cast<float *>(d_tcw_bef);     // read only on the device
        a.p.in_gba = const_cast<uint8_t *>(d_in_gba);
        a.p.origin = nullptr; a.p.child_off = nullptr; a.p.child_kf = nullptr;
        L.send(c.stream);
        if (K) {
            hipLaunchKernelGGL(gba_keyframe_kernel, dim3((unsigned)cdiv(h.n_kf, LC_THREADS)), dim3(LC_THREADS), 0, c.stream, a);
            SIVO_HIP(hipGetLastError());
        }
        if (P) {
            hipLaunchKernelGGL(gba_point_kernel, dim3((unsigned)cdiv(h.n_points, LC_THREADS)), dim3(LC_THREADS), 0, c.stream, a);
            SIVO_HIP(hipGetLastError());
        }
        SIVO_HIP(hipMemcpyAsync(L.host(a.p.tcw_out), a.p.tcw_out, L.results(), hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        const float *ht = L.host(a.p.tcw_out), *ho = L.host(a.p.ow_out), *hp = L.host(a.p.pos_out);
        const uint8_t *hr = L.host(a.p.kf_reached), *hi = L.host(a.in_gba_after), *hs = L.host(a.p.point_status);
        for (size_t k = 0; k < K; ++k) {
            h.kf_reached[k] = hr[k];
            if (!hr[k]) continue;                                       // unreached: everything of the keyframe stays
            if (!h.in_gba[k] && hi[k]) {                                // (:708-710)
                std::memcpy(h.tcw_gba + 16 * k, ht + 16 * k, 64);
                h.in_gba[k] = 1;
            }
            std::memcpy(h.tcw_bef + 16 * k, h.tcw + 16 * k, 64);         // (:715)
            std::memcpy(h.tcw_out + 16 * k, ht + 16 * k, 64);           // (:716)
            std::memcpy(h.ow_out + 3 * k, ho + 3 * k, 12);
        }
        for (size_t p = 0; p < P; ++p) {
            h.point_status[p] = hs[p];
            if (hs[p] == SIVO_GBA_POINT_FROM_BA || hs[p] == SIVO_GBA_POINT_CARRIED) std::memcpy(h.pos_out + 3 * p, hp + 3 * p, 12);
        }
        return SIVO_OK;
    });
}
