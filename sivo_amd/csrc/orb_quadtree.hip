// orb_quadtree.hip — ORBextractor::DistributeOctTree (reference ORBextractor.cc:544-750) on the device: one workgroup distributes
// one candidate set (one pyramid level of one image), a batch is a grid of such workgroups.  The steps and why they equal the host
// routine (orb_host.cpp) byte for byte are in orb_quadtree_math.hpp; this file runs them: a body over n items is a strided loop
// of the workgroup's threads followed by __syncthreads(), a scan is a block scan, the counters are LDS integer atomics whose result
// does not depend on arrival order.  No workgroup waits for or reads anything of another: the grid may be dispatched in any order.
//
// State per workgroup: the cell tables in LDS (QT_MAX_CELLS cells, 56 bytes each: two lists, the quadrant counts, two scan arrays,
// two `grown` lists, the split order and its inverse = 112 KB of the CU's 160 KB, 136 KB with the candidates; a table for 2048 cells is what a 2000-feature
// extractor needs three times over on its largest level), and the candidates: a copy of the packed words and one 16-bit list
// position each, read twice per pass — in LDS too where a set has at most QT_LDS_CANDS of them (24 KB; a level of a 352 x 1024
// frame has up to about 3000), otherwise in device scratch.  A copy in either case: the words usually come from host memory the
// FAST kernel wrote, which a kernel should cross the bus for once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "orb_quadtree.hpp"

namespace sivo {

constexpr int QT_T = 1024;
constexpr int QT_LDS_CANDS = 4096;       // sets up to this size keep their candidates in LDS
static_assert(QT_MAX_CELLS <= 2 * QT_T && QT_MAX_CELLS < QT_NONE, "the block scan takes two items per thread; positions are 16 bits");

struct QtExec {
    uint32_t *wsum;     // QT_T / 64 + 1 words of LDS
    template <class F> __device__ __forceinline__ void each(int n, F f) {
        for (int i = threadIdx.x; i < n; i += QT_T) f(i);
        __syncthreads();
    }
    __device__ __forceinline__ void zero(int32_t *p) { if (threadIdx.x == 0) *p = 0; }
    // exclusive prefix sums of a[0 .. n), n <= 2 * QT_T, in place; the total
    __device__ uint32_t scan(uint32_t *a, int n) {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i0 = 2 * tid;
        const uint32_t v0 = i0 < n ? a[i0] : 0u, v1 = i0 + 1 < n ? a[i0 + 1] : 0u, s = v0 + v1;
        uint32_t x = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        if (tid == 0) {
            uint32_t run = 0;
            for (int w = 0; w < QT_T / 64; ++w) { const uint32_t t = wsum[w]; wsum[w] = run; run += t; }
            wsum[QT_T / 64] = run;
        }
        __syncthreads();
        const uint32_t excl = x - s + wsum[wave], total = wsum[QT_T / 64];
        if (i0 < n) a[i0] = excl;
        if (i0 + 1 < n) a[i0 + 1] = excl + v0;
        __syncthreads();
        return total;
    }
};

__global__ __launch_bounds__(QT_T) void orb_quadtree_kernel(const QtSet *sets, const int32_t *off, int32_t off_limit, const uint32_t *words,
                                                           uint32_t *work_words, uint16_t *work_ids, uint32_t *out_words, int32_t *out_idx,
                                                           int32_t *out_count, int32_t *out_status) {
    __shared__ QtCell s_cells[2][QT_MAX_CELLS];
    __shared__ int32_t s_cnt4[QT_MAX_CELLS][4];
    __shared__ uint32_t s_sc[QT_MAX_CELLS], s_sk[QT_MAX_CELLS];
    __shared__ uint16_t s_grown[2][QT_MAX_CELLS], s_srt[QT_MAX_CELLS], s_rk[QT_MAX_CELLS];
    __shared__ uint32_t s_wsum[QT_T / 64 + 1];
    __shared__ int32_t s_below;
    __shared__ uint32_t s_word[QT_LDS_CANDS];
    __shared__ uint16_t s_cid[QT_LDS_CANDS];
    const int s = blockIdx.x, tid = threadIdx.x;
    const QtSet set = sets[s];
    const int b = off[set.off_b], e = off[set.off_e];
    auto leave = [&](int status, int count) {
        if (tid == 0) { out_count[s] = count; out_status[s] = status; }
    };
    if (b < 0 || e < b || e > off_limit) return leave(QT_ERR_OFFSETS, 0);
    const int n = e - b;
    if (n == 0) return leave(QT_OK, 0);
    uint32_t *const word = n <= QT_LDS_CANDS ? s_word : work_words + b;
    for (int i = tid; i < n; i += QT_T) word[i] = words[b + i];
    __syncthreads();
    QtState S;
    S.word = word; S.cid = n <= QT_LDS_CANDS ? s_cid : work_ids + b; S.n = n;
    S.cur = s_cells[0]; S.nxt = s_cells[1];
    S.cnt4 = s_cnt4; S.sc = s_sc; S.sk = s_sk;
    S.grown = s_grown[0]; S.grown_nxt = s_grown[1];
    S.srt = s_srt; S.rk = s_rk; S.below = &s_below;
    QtExec x{s_wsum};
    int count = 0;
    const int status = qt_distribute(x, S, set, &count);
    if (status != QT_OK) return leave(status, 0);
    if (count > set.slot_count) return leave(QT_ERR_SLOTS, 0);
    for (int j = tid; j < count; j += QT_T) {
        const int best = S.cnt4[j][1];
        out_words[set.slot_base + j] = S.word[best];
        if (out_idx) out_idx[set.slot_base + j] = best;
    }
    leave(QT_OK, count);
}

void quadtree_launch(hipStream_t st, int n_sets, const QtSet *d_sets, const int32_t *off, int32_t off_limit, const uint32_t *words,
                     uint32_t *work_words, uint16_t *work_ids, uint32_t *out_words, int32_t *out_idx, int32_t *out_count,
                     int32_t *out_status) {
    hipLaunchKernelGGL(orb_quadtree_kernel, dim3(n_sets), dim3(QT_T), 0, st, d_sets, off, off_limit, words, work_words, work_ids, out_words,
                       out_idx, out_count, out_status);
}

void quadtree_roots(int w, int h, int *n_ini, float *h_x) {
    *n_ini = (int)std::round((float)w / h);
    *h_x = *n_ini > 0 ? (float)w / *n_ini : 0.f;
}

const char *quadtree_status_text(int status) {
    switch (status) {
    case QT_OK: return "ok";
    case QT_ERR_CELLS: return "the list outgrew the cell table";
    case QT_ERR_ROUNDS: return "the pass limit was reached";
    case QT_ERR_OFFSETS: return "the candidate offsets are inconsistent";
    case QT_ERR_SLOTS: return "the list outgrew its output slots";
    default: return "the kernel left no status";
    }
}

namespace {

// grow-only buffers of sivo_orb_distribute_batch_dev, one set per device, used under one lock
struct BatchBuffers {
    void *dev = nullptr;
    size_t cap = 0;
    void *need(size_t bytes) {
        if (bytes > cap) {
            if (dev) (void)hipFree(dev);
            dev = nullptr; cap = 0;
            SIVO_HIP(hipMalloc(&dev, bytes + bytes / 2));
            cap = bytes + bytes / 2;
        }
        return dev;
    }
};
std::mutex g_batch_mu;
BatchBuffers g_batch[64];

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace
}  // namespace sivo

using namespace sivo;

extern "C" int sivo_orb_distribute_batch_dev(int n_sets, const int64_t *set_off, const SivoKeyPoint *keys, const int32_t *min_x,
                                             const int32_t *max_x, const int32_t *min_y, const int32_t *max_y, const int32_t *n_features,
                                             int64_t out_capacity, SivoKeyPoint *out, int64_t *out_off, int device) {
    return guarded([&] {
        // ---- every refusal, before any device is touched
        if (n_sets < 0) throw std::invalid_argument("n_sets is negative");
        if (n_sets == 0) { if (out_off) out_off[0] = 0; return SIVO_OK; }
        if (!set_off || !out_off || !min_x || !max_x || !min_y || !max_y || !n_features)
            throw std::invalid_argument("a NULL array with n_sets > 0");
        if (set_off[0] != 0) throw std::invalid_argument("set_off does not start at 0");
        for (int s = 0; s < n_sets; ++s)
            if (set_off[s + 1] < set_off[s]) throw std::invalid_argument("set_off decreases at set " + std::to_string(s));
        const int64_t total_in = set_off[n_sets];
        if (total_in > 0 && !keys) throw std::invalid_argument("keys is NULL with " + std::to_string(total_in) + " keys");
        if (out_capacity < 0 || (out_capacity > 0 && !out)) throw std::invalid_argument("out is NULL with out_capacity > 0");
        if (total_in > 0x7fffffff) throw std::invalid_argument("more than 2^31 - 1 keys");
        std::vector<QtSet> sets((size_t)n_sets);
        int64_t slots = 0;
        for (int s = 0; s < n_sets; ++s) {
            const std::string at = " (set " + std::to_string(s) + ")";
            if (max_x[s] <= min_x[s] || max_y[s] <= min_y[s]) throw std::invalid_argument("empty region" + at);
            const int64_t w = (int64_t)max_x[s] - min_x[s], h = (int64_t)max_y[s] - min_y[s];
            if (w > QT_MAX_EXTENT || h > QT_MAX_EXTENT) throw std::invalid_argument("region extents up to 4096 are supported" + at);
            if (n_features[s] < 1) throw std::invalid_argument("n_features < 1" + at);
            QtSet &q = sets[(size_t)s];
            quadtree_roots((int)w, (int)h, &q.n_ini, &q.h_x);
            if (q.n_ini < 1) throw std::invalid_argument("round(W / H) < 1: the region has no root cell" + at);
            q.off_b = s; q.off_e = s + 1; q.w = (int)w; q.h = (int)h; q.target = n_features[s];
        }
        for (int s = 0; s < n_sets; ++s)
            for (int64_t i = set_off[s]; i < set_off[s + 1]; ++i) {
                const SivoKeyPoint &k = keys[i];
                const bool ok = k.x >= 0.f && k.x < (float)sets[(size_t)s].w && k.x == std::floor(k.x) && k.y >= 0.f &&
                                k.y < (float)sets[(size_t)s].h && k.y == std::floor(k.y) && k.response >= 0.f && k.response < 256.f &&
                                k.response == std::floor(k.response);
                if (!ok)
                    throw std::invalid_argument("key " + std::to_string(i - set_off[s]) + " of set " + std::to_string(s) +
                                                ": x, y must be integers inside the region and response an integer in [0, 256)");
            }
        for (int s = 0; s < n_sets; ++s) {
            QtSet &q = sets[(size_t)s];
            const int64_t bound = qt_cell_bound(q.target, q.n_ini);
            if (bound > QT_MAX_CELLS)
                return fail(SIVO_ERR_CAPACITY, "set %d can reach max(n_features + 3, 4 * n_ini) = %lld cells, the kernel's table holds %d", s,
                            (long long)bound, QT_MAX_CELLS);
            // (every cell of a list holds a candidate: never more cells than candidates either)
            q.slot_base = (int)slots; q.slot_count = (int)std::min<int64_t>(bound, set_off[s + 1] - set_off[s]);
            slots += q.slot_count;
        }
        for (int s = 0; s <= n_sets; ++s) out_off[s] = 0;
        if (total_in == 0) return SIVO_OK;                       // only empty sets: no launch
        if (device < 0 || device >= 64 || sivo_device_count() <= device)
            return fail(SIVO_ERR_RUNTIME, "HIP device %d is not available (%d visible): libsivo_hip has no CPU fallback", device,
                        sivo_device_count());
        // ---- one upload, one launch, one download
        const size_t N = (size_t)total_in, S = (size_t)n_sets, K = (size_t)slots;
        const size_t o_sets = 0, o_off = align256(o_sets + S * sizeof(QtSet)), o_words = align256(o_off + (S + 1) * 4),
                     o_end_in = align256(o_words + N * 4), o_work = o_end_in, o_ids = align256(o_work + N * 4),
                     o_res = align256(o_ids + N * 2), o_count = o_res, o_status = o_count + S * 4, o_kw = align256(o_status + S * 4),
                     o_ki = align256(o_kw + K * 4), o_end = align256(o_ki + K * 4);
        std::vector<uint8_t> stage(o_end_in, 0);
        std::memcpy(stage.data() + o_sets, sets.data(), S * sizeof(QtSet));
        int32_t *h_off = reinterpret_cast<int32_t *>(stage.data() + o_off);
        for (size_t s = 0; s <= S; ++s) h_off[s] = (int32_t)set_off[s];
        uint32_t *h_words = reinterpret_cast<uint32_t *>(stage.data() + o_words);
        for (size_t i = 0; i < N; ++i)
            h_words[i] = (uint32_t)keys[i].x | ((uint32_t)keys[i].y << 12) | ((uint32_t)keys[i].response << 24);
        std::vector<uint8_t> res(o_end - o_res);
        {
            DeviceGuard dg(device);
            std::lock_guard<std::mutex> one(g_batch_mu);
            uint8_t *d = static_cast<uint8_t *>(g_batch[device].need(o_end));
            SIVO_HIP(hipMemcpy(d, stage.data(), o_end_in, hipMemcpyHostToDevice));
            SIVO_HIP(hipMemset(d + o_res, 0xff, o_end - o_res));                    // (status -1: the kernel left none)
            quadtree_launch(nullptr, n_sets, reinterpret_cast<const QtSet *>(d + o_sets), reinterpret_cast<const int32_t *>(d + o_off),
                            (int32_t)total_in, reinterpret_cast<const uint32_t *>(d + o_words), reinterpret_cast<uint32_t *>(d + o_work),
                            reinterpret_cast<uint16_t *>(d + o_ids), reinterpret_cast<uint32_t *>(d + o_kw),
                            reinterpret_cast<int32_t *>(d + o_ki), reinterpret_cast<int32_t *>(d + o_count),
                            reinterpret_cast<int32_t *>(d + o_status));
            SIVO_HIP(hipGetLastError());
            SIVO_HIP(hipMemcpy(res.data(), d + o_res, o_end - o_res, hipMemcpyDeviceToHost));
        }
        const int32_t *count = reinterpret_cast<const int32_t *>(res.data()), *status = count + S;
        const int32_t *kept = reinterpret_cast<const int32_t *>(res.data() + (o_ki - o_res));
        for (size_t s = 0; s < S; ++s)
            if (status[s] != QT_OK || count[s] < 0 || count[s] > sets[s].slot_count)
                return fail(SIVO_ERR_RUNTIME, "device quadtree, set %zu: %s (status %d)", s, quadtree_status_text(status[s]), status[s]);
        for (size_t s = 0; s < S; ++s) out_off[s + 1] = out_off[s] + count[s];
        if (out_off[S] > out_capacity)
            return fail(SIVO_ERR_CAPACITY, "%lld keypoints, capacity %lld", (long long)out_off[S], (long long)out_capacity);
        for (size_t s = 0; s < S; ++s)
            for (int32_t j = 0; j < count[s]; ++j) {
                const int32_t i = kept[sets[s].slot_base + j];
                if (i < 0 || i >= set_off[s + 1] - set_off[s]) return fail(SIVO_ERR_RUNTIME, "device quadtree, set %zu: kept index %d outside the set", s, i);
                out[out_off[s] + j] = keys[set_off[s] + i];
            }
        return SIVO_OK;
    });
}
