// localmap_handle.hpp — what localmap.hip, ba_window.hip and localmap_track.hip share: the resident map's handle with its attribute
// store, the solver context its calls run on, the argument block of the point passes (localmap_first / _count / _scatter_kernel, defined
// in localmap.hip), the workgroup scans and the device part of sivo_localmap_update as a function (lm_run_update).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.hpp"
#include "solver_host.hpp"

#include "localmap_math.hpp"
#include "localmap_delta_math.hpp"
#include "localmap_track_math.hpp"

namespace sivo {

constexpr int LP_THREADS = 256;

enum { LM_HDR_VOTED = 0, LM_HDR_N_KF, LM_HDR_REF, LM_HDR_N_POINTS, LM_HDR_N_LIST, LM_HDR_G, LM_HDR_WORDS = 8 };

struct LmCall {
    SivoLocalMapTables t;          // device pointers; kf_order is never null here
    uint32_t *first;               // n_points, the handle's; LM_FIRST_NONE everywhere before the select kernel
    int n_slots, n_kf_pre, n_pt_pre, n_prev, point_cap;
    const int32_t *frame_point, *kf_pre, *pt_pre, *prev;
    uint32_t *marks_g;             // one bit per keyframe, zeroed: the marks where n_kf > SIVO_COVIS_LDS_KF
    int32_t *counts;               // n_kf, zeroed
    int32_t *hdr;                  // LM_HDR_*
    uint8_t *slot_cleared;         // n_slots
    int32_t *local_kf;             // n_kf
    int32_t *local_point;          // point_cap
    int32_t *list_off;             // max(n_kf, n_prev) + 1
    int32_t *block_sum;            // one per block of the point kernels
};

// The exclusive prefix of v over the workgroup and its total; wave_tot holds one entry per wave.  Every thread of the workgroup calls it.
template <int THREADS>
__device__ inline int32_t lm_block_excl_scan(int32_t v, int32_t *wave_tot, int32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    int32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        const int32_t x = wave_tot[w];
        if (w < wave) before += x;
        total += x;
    }
    __syncthreads();
    return before + inc - v;
}

// x[0] + .. + x[n - 1], the same in every thread of a workgroup of LP_THREADS
__device__ inline int32_t lm_block_sum(const int32_t *x, int n, int32_t *acc) {
    if (threadIdx.x == 0) *acc = 0;
    __syncthreads();
    int32_t s = 0;
    for (int i = threadIdx.x; i < n; i += LP_THREADS) s += x[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(acc, s);
    __syncthreads();
    const int32_t r = *acc;
    __syncthreads();
    return r;
}

// ---- the point passes: the bodies of localmap_first / _count / _scatter_kernel, which ba_window.hip launches under its own names ------
// They walk the slot sequence of the list hdr names (local_kf where LM_HDR_VOTED, else prev): LM_HDR_N_LIST keyframes, LM_HDR_G slots,
// list_off their exclusive prefix; first[] is LM_FIRST_NONE or LM_FIRST_PREMARKED before pass 1.  Workgroups of LP_THREADS.
struct LmList {
    const int32_t *list;
    int32_t n, G;
};

__device__ inline LmList lm_list(const LmCall &a) {
    LmList l;
    l.list = a.hdr[LM_HDR_VOTED] ? a.local_kf : a.prev;
    l.n = a.hdr[LM_HDR_N_LIST];
    l.G = a.hdr[LM_HDR_G];
    return l;
}

// pass 1 over the slot sequence g: atomicMin(first[p], g + 1)
__device__ inline void lm_first_pass(const LmCall &a) {
    const LmList l = lm_list(a);
    const int64_t g = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if (g >= l.G) return;
    const int32_t p = lm_slot_point(a.t, l.list, a.list_off, l.n, (int32_t)g);
    if (p >= 0) atomicMin(&a.first[p], (uint32_t)g + 1u);
}

// pass 2a: how many slots of each block of 256 push their point
__device__ inline void lm_count_pass(const LmCall &a) {
    __shared__ int32_t wave_n[LP_THREADS / 64];
    const LmList l = lm_list(a);
    const int64_t g = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    if ((int64_t)blockIdx.x * LP_THREADS >= l.G) return;               // the whole block
    bool keep = false;
    if (g < l.G) keep = lm_point_survives(a.t, a.first, lm_slot_point(a.t, l.list, a.list_off, l.n, (int32_t)g), (int32_t)g);
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

// pass 2b: exclusive scan inside the block, the sum of the blocks before it, the scatter in order
__device__ inline void lm_scatter_pass(const LmCall &a) {
    __shared__ int32_t wave_tot[LP_THREADS / 64];
    __shared__ int32_t acc;
    const LmList l = lm_list(a);
    const int nb = (int)(((int64_t)l.G + LP_THREADS - 1) / LP_THREADS);
    const int blk = blockIdx.x;
    if (blk >= nb && blk != 0) return;                                  // the whole block; block 0 stays for the count
    const int64_t g = (int64_t)blk * LP_THREADS + threadIdx.x;
    int32_t p = -1;
    bool keep = false;
    if (g < l.G) {
        p = lm_slot_point(a.t, l.list, a.list_off, l.n, (int32_t)g);
        keep = lm_point_survives(a.t, a.first, p, (int32_t)g);
    }
    int32_t total;
    const int32_t excl = lm_block_excl_scan<LP_THREADS>(keep ? 1 : 0, wave_tot, total);
    const int32_t base = lm_block_sum(a.block_sum, blk, &acc);
    if (keep && base + excl < a.point_cap) a.local_point[base + excl] = p;     // (:1119)
    if (blk == 0) {
        const int32_t all = lm_block_sum(a.block_sum, nb, &acc);
        if (threadIdx.x == 0) a.hdr[LM_HDR_N_POINTS] = all;
    }
}

inline void lm_throw(const char *what, const char *e) {
    if (e) throw std::invalid_argument(std::string(what) + ": " + e);
}

inline SolverCtx &lm_ctx() {
    static thread_local SolverCtx c(false, 1 << 20, 0, 1 << 20);
    c.bind();
    return c;
}

// What a caller of lm_run_update adds to the update: regions of the call's one upload, and launches behind the point passes on the
// call's stream, before the download and the call's one synchronisation.
struct LmUpdateHook {
    virtual void regions(Layout &L) = 0;
    virtual void launch(const LmCall &a, hipStream_t stream) = 0;
    virtual ~LmUpdateHook() {}
};

// the arguments of sivo_localmap_update
struct LmUpdateArgs {
    int n_slots; const int32_t *frame_point; int n_kf_premarked; const int32_t *kf_premarked; int n_point_premarked;
    const int32_t *point_premarked; int n_prev; const int32_t *prev_local_kf; int32_t *voted; uint8_t *slot_cleared; int kf_capacity;
    int32_t *local_kf, *n_local_kf, *ref_kf; int point_capacity; int32_t *local_point, *n_local_points, *counts;
};

}  // namespace sivo

struct sivo_localmap;
namespace sivo {
// sivo_localmap_update on a handle whose mutex the caller holds, the arguments checked (g_prev from lm_check_update): the upload, the
// five launches, the hook's, the download, the synchronisation, the outputs.  `who` heads the text of SIVO_ERR_CAPACITY.  `call`
// receives the call's device pointers, which stay valid on this thread until its next call on a handle.  Defined in localmap.hip.
int lm_run_update(sivo_localmap *m, const LmUpdateArgs &u, int64_t g_prev, const char *who, LmUpdateHook *hook, LmCall *call);
}  // namespace sivo

struct sivo_localmap {
    std::mutex mu;
    int device = -1;
    sivo::DeviceBuf buf_a{1 << 20}, buf_b{1 << 20};            // the tables and first[] live in dev(cur), apply builds into the other; grow-only
    sivo::DeviceBuf &dev(int i) { return i ? buf_b : buf_a; }
    int cur = 0;
    int64_t total[sivo::LMD_TABLES] = {0, 0, 0, 0};            // the entries of obs_kf, slot_point, covis_kf, child_kf
    SivoLocalMapTables d{};                // device pointers
    uint32_t *first = nullptr;
    std::vector<int64_t> slot_off;         // host copy: the slot counts bound the grids and size prev_local_kf's walk
    int64_t total_slots = 0;

    // ---- the attribute store (sivo_localmap_set_points): structure-of-arrays over the handle's point indices, in an allocation of its
    // own (the tables ping-pong between buf_a and buf_b), which grows by a device copy and keeps every stored row
    char *attr_base = nullptr;
    size_t attr_cap = 0;                   // rows; a multiple of 64, so every array starts at a multiple of 256 bytes
    sivo::LtAttrs attr{};                  // device pointers into attr_base
    std::vector<uint64_t> attr_set;        // one bit per point: a set_points named it since create / replace / its append
    int64_t n_attr_set = 0;

    static sivo::LtAttrs attr_at(char *base, size_t cap) {
        sivo::LtAttrs a;
        a.pos = (float *)base; a.normal = (float *)(base + 12 * cap); a.min_dist = (float *)(base + 24 * cap);
        a.max_dist = (float *)(base + 28 * cap); a.desc = (uint32_t *)(base + 32 * cap); a.n_obs = (int32_t *)(base + 64 * cap);
        return a;
    }
    // room for n_points rows; the first `keep` rows survive a growth (copied on `stream`, which is synchronised before the old
    // allocation is freed)
    void attr_reserve(size_t n_points, size_t keep, hipStream_t stream) {
        if (n_points <= attr_cap) return;
        const size_t cap = (std::max<size_t>(2 * n_points, 4096) + 63) / 64 * 64;
        char *base = nullptr;
        SIVO_HIP(hipMalloc((void **)&base, sivo::LT_ROW_BYTES * cap));
        const sivo::LtAttrs n = attr_at(base, cap);
        try {
            if (keep && attr_base) {
                SIVO_HIP(hipMemcpyAsync(n.pos, attr.pos, 12 * keep, hipMemcpyDeviceToDevice, stream));
                SIVO_HIP(hipMemcpyAsync(n.normal, attr.normal, 12 * keep, hipMemcpyDeviceToDevice, stream));
                SIVO_HIP(hipMemcpyAsync(n.min_dist, attr.min_dist, 4 * keep, hipMemcpyDeviceToDevice, stream));
                SIVO_HIP(hipMemcpyAsync(n.max_dist, attr.max_dist, 4 * keep, hipMemcpyDeviceToDevice, stream));
                SIVO_HIP(hipMemcpyAsync(n.desc, attr.desc, 32 * keep, hipMemcpyDeviceToDevice, stream));
                SIVO_HIP(hipMemcpyAsync(n.n_obs, attr.n_obs, 4 * keep, hipMemcpyDeviceToDevice, stream));
                SIVO_HIP(hipStreamSynchronize(stream));
            }
        } catch (...) {
            (void)hipFree(base);
            throw;
        }
        if (attr_base) (void)hipFree(attr_base);
        attr_base = base; attr_cap = cap; attr = n;
    }
    // the bitmap for n_points rows: the rows it already holds keep their bit, new rows are unset
    void attr_resize(size_t n_points) { attr_set.resize((n_points + 63) / 64, 0); }
    void attr_unset_all(size_t n_points) {
        attr_set.assign((n_points + 63) / 64, 0);
        n_attr_set = 0;
    }
    bool attr_is_set(int32_t p) const { return (attr_set[(size_t)p >> 6] >> (p & 63)) & 1u; }
    void attr_release() {
        if (attr_base) (void)hipFree(attr_base);
        attr_base = nullptr; attr_cap = 0;
    }
};
