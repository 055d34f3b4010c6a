// ba_window.hip — the window of Optimizer::LocalBundleAdjustment (reference src/orbslam/Optimizer.cc:496-559: lLocalKeyFrames,
// lLocalMapPoints, lFixedKFs; :585-622: the vertices; :651-670: one edge per observation) on the resident map of localmap.hip:
// sivo_localmap_ba_window.  The per-item bodies and the argument check are ba_window_math.hpp; everything is integer and no result
// depends on the order in which atomics arrive (minima and adds only).  One upload of the call's four lists, one memset of first[],
// twelve launches, the 64-byte header back and a synchronisation, then the six result arrays at their exact sizes and a second one.
//
// bawin_select_kernel       ONE workgroup: kf_first = BW_FIRST_NONE and pose_of = -1 everywhere, then BW_FIRST_MARKED on every
//                           candidate and premarked keyframe and LM_FIRST_PREMARKED on every premarked point; the candidates that are
//                           listed (:499, :510-512) compacted in order, a ballot per wave and a prefix over the waves, into local_kf and
//                           pose_of; the exclusive prefix of their slot counts (list_off).
// bawin_point_*_kernel      lLocalMapPoints (:516-533): the three point passes of sivo_localmap_update (localmap_handle.hpp).
// bawin_len / _scan_kernel  <0>: the exclusive prefix of the local points' observation rows (row_off) and their total H.
// bawin_fixed_*_kernel      lFixedKFs (:537-559), the same three passes over the observation sequence h: atomicMin(kf_first[k], h + 1),
//                           the survivors of each block of 256, the ordered scatter into fixed_kf and pose_of.
// bawin_len / _scan_kernel  <1>: the observations of each local point that become edges, their exclusive prefix (edge_off).
// bawin_edge_kernel         one wave per observation that becomes an edge: lane e reads the entries e, e + 64, ... of the keyframe's
//                           slot row; a ballot per chunk gives the number of slots that hold the point and the lowest of them.
//
// The list lengths stay on the device between the launches (hdr); the grids are sized from bounds the host knows: the handle's slot
// total (no keyframe is listed twice), min(points, slots) and the handle's observation total (no point is listed twice).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <stdexcept>

#include "localmap_handle.hpp"

#include "ba_window_math.hpp"

namespace sivo {

constexpr int BW_THREADS = 1024;

enum { BW_HDR_H = LM_HDR_WORDS, BW_HDR_N_FIXED, BW_HDR_N_EDGES, BW_HDR_WORDS = 16 };

struct BwCall {
    LmCall p;                      // what the point passes read and write: t, first, hdr, local_kf, list_off, block_sum, local_point, point_cap
    int n_cand, n_kl_pre, n_kx_pre, n_pt_pre;
    const int32_t *cand, *kl_pre, *kx_pre, *pt_pre;
    uint32_t *kf_first;            // n_kf
    int32_t *pose_of;              // n_kf
    int32_t *row_off;              // point_cap + 1
    int32_t *fixed_kf;             // n_kf
    int32_t *block_sum;            // one per block of the passes over the local points and over their observations
    int64_t *edge_off;             // point_cap + 1
    int32_t *edge_pose, *edge_slot;        // the handle's observation total
};

__global__ __launch_bounds__(BW_THREADS) void bawin_select_kernel(BwCall a) {
    __shared__ int32_t wave_tot[BW_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < a.p.t.n_kf; k += BW_THREADS) {
        a.kf_first[k] = BW_FIRST_NONE;
        a.pose_of[k] = -1;
    }
    __syncthreads();
    for (int i = tid; i < a.n_cand; i += BW_THREADS) a.kf_first[a.cand[i]] = BW_FIRST_MARKED;             // (:500, :508)
    for (int i = tid; i < a.n_kl_pre; i += BW_THREADS) a.kf_first[a.kl_pre[i]] = BW_FIRST_MARKED;
    for (int i = tid; i < a.n_kx_pre; i += BW_THREADS) a.kf_first[a.kx_pre[i]] = BW_FIRST_MARKED;
    for (int i = tid; i < a.n_pt_pre; i += BW_THREADS) a.p.first[a.pt_pre[i]] = LM_FIRST_PREMARKED;

    // ---- lLocalKeyFrames (:499, :506-513): the listed candidates in order; n is the same in every thread
    int32_t n = 0;
    for (int base = 0; base < a.n_cand; base += BW_THREADS) {
        const int i = base + tid;
        const bool take = i < a.n_cand && bw_cand_listed(a.p.t, a.cand, i);
        const unsigned long long b = __ballot(take);
        const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = __popcll(b);
        __syncthreads();
        int32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < BW_THREADS / 64; ++w) {
            const int32_t x = wave_tot[w];
            if (w < wave) before += x;
            total += x;
        }
        if (take) {
            a.p.local_kf[n + before + in_wave] = a.cand[i];
            a.pose_of[a.cand[i]] = n + before + in_wave;                // (:585-605)
        }
        n += total;
        __syncthreads();
    }

    // ---- what the point passes walk
    int32_t run = 0;
    for (int base = 0; base < n; base += BW_THREADS) {
        const int i = base + tid;
        int32_t cnt = 0;
        if (i < n) cnt = (int32_t)(a.p.t.slot_off[a.p.local_kf[i] + 1] - a.p.t.slot_off[a.p.local_kf[i]]);
        int32_t total;
        const int32_t excl = lm_block_excl_scan<BW_THREADS>(cnt, wave_tot, total);
        if (i < n) a.p.list_off[i] = run + excl;
        run += total;
    }
    if (tid == 0) {
        a.p.list_off[n] = run;
        a.p.hdr[LM_HDR_VOTED] = 1;                                      // the point passes walk local_kf
        a.p.hdr[LM_HDR_N_KF] = n;
        a.p.hdr[LM_HDR_N_LIST] = n;
        a.p.hdr[LM_HDR_G] = run;
    }
}

__global__ __launch_bounds__(LP_THREADS) void bawin_point_first_kernel(BwCall a) { lm_first_pass(a.p); }
__global__ __launch_bounds__(LP_THREADS) void bawin_point_count_kernel(BwCall a) { lm_count_pass(a.p); }
__global__ __launch_bounds__(LP_THREADS) void bawin_point_scatter_kernel(BwCall a) { lm_scatter_pass(a.p); }

// MODE 0: the observations of local point i; MODE 1: those that become edges
template <int MODE>
__device__ inline int32_t bw_len(const BwCall &a, int32_t i) {
    const int32_t len = bw_row_len(a.p.t, a.p.local_point, i);
    return MODE == 0 ? len : bw_kept_before(a.p.t, a.pose_of, a.p.local_point[i], len);
}

// pass a of an offset array over the local points: the lengths of a block of LP_THREADS, summed
template <int MODE>
__global__ __launch_bounds__(LP_THREADS) void bawin_len_kernel(BwCall a) {
    __shared__ int32_t wave_tot[LP_THREADS / 64];
    const int32_t n = a.p.hdr[LM_HDR_N_POINTS];
    if ((int64_t)blockIdx.x * LP_THREADS >= n) return;                 // the whole block
    const int64_t i = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    int32_t total;
    (void)lm_block_excl_scan<LP_THREADS>(i < n ? bw_len<MODE>(a, (int32_t)i) : 0, wave_tot, total);
    if (threadIdx.x == 0) a.block_sum[blockIdx.x] = total;
}

// pass b: the exclusive scan inside the block and the sum of the blocks before it; the last point writes the total
template <int MODE>
__global__ __launch_bounds__(LP_THREADS) void bawin_scan_kernel(BwCall a) {
    __shared__ int32_t wave_tot[LP_THREADS / 64];
    __shared__ int32_t acc;
    const int32_t n = a.p.hdr[LM_HDR_N_POINTS];
    const int blk = blockIdx.x;
    auto store = [&](int32_t i, int32_t v) {
        if (MODE == 0) a.row_off[i] = v;
        else a.edge_off[i] = v;
    };
    if (n == 0) {
        if (blk == 0 && threadIdx.x == 0) {
            store(0, 0);
            a.p.hdr[MODE == 0 ? BW_HDR_H : BW_HDR_N_EDGES] = 0;
        }
        return;
    }
    if ((int64_t)blk * LP_THREADS >= n) return;                         // the whole block
    const int64_t i = (int64_t)blk * LP_THREADS + threadIdx.x;
    const int32_t len = i < n ? bw_len<MODE>(a, (int32_t)i) : 0;
    int32_t total;
    const int32_t excl = lm_block_excl_scan<LP_THREADS>(len, wave_tot, total);
    const int32_t base = lm_block_sum(a.block_sum, blk, &acc);
    if (i < n) store((int32_t)i, base + excl);
    if (i == n - 1) {
        store(n, base + excl + len);
        a.p.hdr[MODE == 0 ? BW_HDR_H : BW_HDR_N_EDGES] = base + excl + len;
    }
}

// pass 1 over the observation sequence h: atomicMin(kf_first[k], h + 1)
__global__ __launch_bounds__(LP_THREADS) void bawin_fixed_first_kernel(BwCall a) {
    const int64_t h = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (h >= a.p.hdr[BW_HDR_H]) return;
    const BwObs o = bw_obs(a.p.t, a.p.local_point, a.row_off, a.p.hdr[LM_HDR_N_POINTS], (int32_t)h);
    atomicMin(&a.kf_first[o.k], (uint32_t)h + 1u);
}

// pass 2a: how many observations of each block of 256 push their keyframe
__global__ __launch_bounds__(LP_THREADS) void bawin_fixed_count_kernel(BwCall a) {
    __shared__ int32_t wave_n[LP_THREADS / 64];
    const int32_t H = a.p.hdr[BW_HDR_H];
    const int64_t h = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if ((int64_t)blockIdx.x * LP_THREADS >= H) return;                 // the whole block
    bool keep = false;
    if (h < H) keep = bw_fixed_survives(a.p.t, a.kf_first, bw_obs(a.p.t, a.p.local_point, a.row_off, a.p.hdr[LM_HDR_N_POINTS], (int32_t)h).k, (int32_t)h);
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t s = 0;
#pragma unroll
        for (int w = 0; w < LP_THREADS / 64; ++w) s += wave_n[w];
        a.block_sum[blockIdx.x] = s;
    }
}

// pass 2b: the scatter in order; a fixed keyframe's vertex stands behind the local ones (:607-622)
__global__ __launch_bounds__(LP_THREADS) void bawin_fixed_scatter_kernel(BwCall a) {
    __shared__ int32_t wave_tot[LP_THREADS / 64];
    __shared__ int32_t acc;
    const int32_t H = a.p.hdr[BW_HDR_H];
    const int nb = (int)(((int64_t)H + LP_THREADS - 1) / LP_THREADS);
    const int blk = blockIdx.x;
    if (blk >= nb && blk != 0) return;                                  // the whole block; block 0 stays for the count
    const int64_t h = (int64_t)blk * LP_THREADS + threadIdx.x;
    int32_t k = -1;
    bool keep = false;
    if (h < H) {
        k = bw_obs(a.p.t, a.p.local_point, a.row_off, a.p.hdr[LM_HDR_N_POINTS], (int32_t)h).k;
        keep = bw_fixed_survives(a.p.t, a.kf_first, k, (int32_t)h);
    }
    int32_t total;
    const int32_t excl = lm_block_excl_scan<LP_THREADS>(keep ? 1 : 0, wave_tot, total);
    const int32_t base = lm_block_sum(a.block_sum, blk, &acc);
    if (keep) {
        a.fixed_kf[base + excl] = k;                                    // (:555)
        a.pose_of[k] = a.p.hdr[LM_HDR_N_KF] + base + excl;
    }
    if (blk == 0) {
        const int32_t all = lm_block_sum(a.block_sum, nb, &acc);
        if (threadIdx.x == 0) a.p.hdr[BW_HDR_N_FIXED] = all;
    }
}

// one wave per observation h; the waves of those that become no edge leave at once
__global__ __launch_bounds__(LP_THREADS) void bawin_edge_kernel(BwCall a) {
    const int64_t h = (int64_t)blockIdx.x * (LP_THREADS / 64) + (threadIdx.x >> 6);
    if (h >= a.p.hdr[BW_HDR_H]) return;
    const int lane = threadIdx.x & 63;
    const BwObs o = bw_obs(a.p.t, a.p.local_point, a.row_off, a.p.hdr[LM_HDR_N_POINTS], (int32_t)h);
    if (!bw_edge_kept(a.p.t, a.pose_of, o.k)) return;                   // (:670)
    const int64_t e = a.edge_off[o.i] + bw_kept_before(a.p.t, a.pose_of, o.p, o.r);
    const int32_t len = (int32_t)(a.p.t.slot_off[o.k + 1] - a.p.t.slot_off[o.k]);
    int32_t hits = 0, lowest = -1;
    for (int32_t base = 0; base < len; base += 64) {
        const int32_t s = base + lane;
        const unsigned long long b = __ballot(s < len && bw_slot_hit(a.p.t, o.k, s, o.p));
        if (b) {
            if (!hits) lowest = base + __ffsll(b) - 1;
            hits += __popcll(b);
        }
    }
    if (lane == 0) {
        a.edge_pose[e] = a.pose_of[o.k];
        a.edge_slot[e] = bw_slot_code(hits, lowest);
    }
}

}  // namespace sivo

using namespace sivo;

extern "C" int sivo_localmap_ba_window(sivo_localmap_t m, int n_cand, const int32_t *cand_kf, int n_kf_local_pre, const int32_t *kf_local_pre,
                                       int n_kf_fixed_pre, const int32_t *kf_fixed_pre, int n_point_pre, const int32_t *point_pre, int kf_capacity,
                                       int32_t *local_kf, int32_t *fixed_kf, int point_capacity, int32_t *local_point, int64_t *edge_off,
                                       int64_t edge_capacity, int32_t *edge_pose, int32_t *edge_slot, int64_t counts[4]) {
    return guarded([&] {
        if (!m) throw std::invalid_argument("sivo_localmap_ba_window: null handle");
        std::lock_guard<std::mutex> lock(m->mu);
        lm_throw("sivo_localmap_ba_window",
                 bw_check_window(m->d.n_kf, m->d.n_points, m->total_slots, m->total[LMD_OBS], n_cand, cand_kf, n_kf_local_pre, kf_local_pre, n_kf_fixed_pre,
                                 kf_fixed_pre, n_point_pre, point_pre, kf_capacity, local_kf, fixed_kf, point_capacity, local_point, edge_off,
                                 edge_capacity, edge_pose, edge_slot, counts));
        require_device();
        DeviceGuard dg(m->device);
        SolverCtx &c = lm_ctx();
        const size_t K = (size_t)m->d.n_kf, P = (size_t)m->d.n_points, C = (size_t)n_cand;
        const size_t p_max = (size_t)std::min<int64_t>((int64_t)P, m->total_slots);     // no more local points than points, or slots
        const size_t o_max = (size_t)m->total[LMD_OBS];                                 // no more observations of them than observations
        const unsigned nb_slot = (unsigned)std::max<int64_t>(1, cdiv64(m->total_slots, LP_THREADS));
        const unsigned nb_point = (unsigned)std::max<int64_t>(1, cdiv64((int64_t)p_max, LP_THREADS));
        const unsigned nb_obs = (unsigned)std::max<int64_t>(1, cdiv64((int64_t)o_max, LP_THREADS));
        const unsigned nb_wave = (unsigned)std::max<int64_t>(1, cdiv64((int64_t)o_max, LP_THREADS / 64));
        BwCall a{};
        a.p.t = m->d; a.p.first = m->first; a.p.point_cap = (int)p_max;
        a.n_cand = n_cand; a.n_kl_pre = n_kf_local_pre; a.n_kx_pre = n_kf_fixed_pre; a.n_pt_pre = n_point_pre;
        Layout L;
        L.copy(a.cand, cand_kf, 4 * C); L.copy(a.kl_pre, kf_local_pre, 4 * (size_t)n_kf_local_pre);
        L.copy(a.kx_pre, kf_fixed_pre, 4 * (size_t)n_kf_fixed_pre); L.copy(a.pt_pre, point_pre, 4 * (size_t)n_point_pre);
        L.take(a.p.hdr, 4 * BW_HDR_WORDS); L.take(a.p.local_kf, 4 * C); L.take(a.fixed_kf, 4 * K); L.take(a.p.local_point, 4 * p_max);
        L.take(a.edge_off, 8 * (p_max + 1)); L.take(a.edge_pose, 4 * o_max); L.take(a.edge_slot, 4 * o_max);
        L.take(a.kf_first, 4 * K); L.take(a.pose_of, 4 * K); L.take(a.row_off, 4 * (p_max + 1)); L.take(a.p.list_off, 4 * (C + 1));     // scratch
        L.take(a.p.block_sum, 4 * (size_t)nb_slot); L.take(a.block_sum, 4 * (size_t)std::max(nb_point, nb_obs));
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        L.send(c.stream);
        if (P) SIVO_HIP(hipMemsetAsync(m->first, 0xFF, 4 * P, c.stream));
        hipLaunchKernelGGL(bawin_select_kernel, dim3(1), dim3(BW_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(bawin_point_first_kernel, dim3(nb_slot), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(bawin_point_count_kernel, dim3(nb_slot), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(bawin_point_scatter_kernel, dim3(nb_slot), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(bawin_len_kernel<0>, dim3(nb_point), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(bawin_scan_kernel<0>, dim3(nb_point), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(bawin_fixed_first_kernel, dim3(nb_obs), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(bawin_fixed_count_kernel, dim3(nb_obs), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(bawin_fixed_scatter_kernel, dim3(nb_obs), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(bawin_len_kernel<1>, dim3(nb_point), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(bawin_scan_kernel<1>, dim3(nb_point), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(bawin_edge_kernel, dim3(nb_wave), dim3(LP_THREADS), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipMemcpyAsync(L.host(a.p.hdr), a.p.hdr, 4 * BW_HDR_WORDS, hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        const int32_t *hdr = L.host(a.p.hdr);
        const int32_t nl = hdr[LM_HDR_N_KF], np = hdr[LM_HDR_N_POINTS], nf = hdr[BW_HDR_N_FIXED], ne = hdr[BW_HDR_N_EDGES];
        counts[0] = nl; counts[1] = np; counts[2] = nf; counts[3] = ne;
        if (nl > kf_capacity || nf > kf_capacity)
            return fail(SIVO_ERR_CAPACITY, "sivo_localmap_ba_window: %d local and %d fixed keyframes, capacity %d", nl, nf, kf_capacity);
        if (np > point_capacity) return fail(SIVO_ERR_CAPACITY, "sivo_localmap_ba_window: %d local map points, capacity %d", np, point_capacity);
        if (ne > edge_capacity) return fail(SIVO_ERR_CAPACITY, "sivo_localmap_ba_window: %d edges, capacity %lld", ne, (long long)edge_capacity);
        auto down = [&](const void *dev, size_t bytes) {
            if (bytes) SIVO_HIP(hipMemcpyAsync(L.host((const char *)dev), dev, bytes, hipMemcpyDeviceToHost, c.stream));
        };
        down(a.p.local_kf, 4 * (size_t)nl); down(a.fixed_kf, 4 * (size_t)nf); down(a.p.local_point, 4 * (size_t)np);
        down(a.edge_off, 8 * ((size_t)np + 1)); down(a.edge_pose, 4 * (size_t)ne); down(a.edge_slot, 4 * (size_t)ne);
        SIVO_HIP(hipStreamSynchronize(c.stream));
        if (nl) std::memcpy(local_kf, L.host(a.p.local_kf), 4 * (size_t)nl);
        if (nf) std::memcpy(fixed_kf, L.host(a.fixed_kf), 4 * (size_t)nf);
        if (np) std::memcpy(local_point, L.host(a.p.local_point), 4 * (size_t)np);
        std::memcpy(edge_off, L.host(a.edge_off), 8 * ((size_t)np + 1));
        if (ne) std::memcpy(edge_pose, L.host(a.edge_pose), 4 * (size_t)ne);
        if (ne) std::memcpy(edge_slot, L.host(a.edge_slot), 4 * (size_t)ne);
        return SIVO_OK;
    });
}
