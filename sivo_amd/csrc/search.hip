// search.hip — guided matching on CDNA4: the Search* / Fuse members of SIVO::ORBmatcher from the projected point on
// (reference src/orbslam/ORBmatcher.cc:44-127, 161-284, 286-399, 508-629, 631-785, 787-1053, 1055-1276, 1278-1543) and
// the frame grid they query (reference src/orbslam/Frame.cc:205-221, 326-390).
//
// Integer / latency-bound work: a frame holds <= a few thousand 32-byte descriptors (64 KB), a call runs <= a few
// thousand queries with 10-100 candidates each.  One wave per query: the grid cells a window covers are contiguous per
// grid column in a CSR laid out column-major like the reference's mGrid[ix][iy] walk, so a window is <= 2r/16+2 spans
// that the 64 lanes stride over (coalesced index loads, 2 x 16-byte descriptor loads per candidate, v_bcnt for the
// distance, wave-butterfly for best / second best on a (distance, visiting order) key, which reproduces the
// reference's first-minimum-wins scans bit for bit).  The frame's view, the window walk and the key are mframe.hpp's (MframeView,
// scan_window, match_key), the grid arithmetic and Fuse's chi-square gate grid_math.hpp's: fuse_batch.hip runs the same ones.  The host
// side stages through Layout (solver_host.hpp): frame_layout for a frame's arrays at the head of its slab, engine_layout for a call.
//
// Sequential semantics.  In the reference, iteration i of a routine skips keypoints matched by iterations < i.  Here all
// queries run at once against the initial state ("round 0"); accepted picks are registered with atomics, and only if
// two accepted queries picked the same keypoint do repair rounds follow, in which query i excludes the keypoints
// picked in the previous round by BLOCKING queries < i.  By induction query i is final after round i; the loop ends at
// the first round that changes nothing, whose state satisfies the sequential recurrence and is therefore the
// reference's result.  Typical calls end after round 0 (one launch + one 8-byte read-back).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "common.hpp"
#include "frustum_math.hpp"
#include "mframe.hpp"
#include "search_engine.hpp"
#include "solver_host.hpp"

#define SIVO_HISTO 30       // ORBmatcher::HISTO_LENGTH

namespace sivo {
namespace {

struct SearchArgs {
    MframeView V;                // train frame
    // queries
    int nq;
    const SivoSearchQuery *q;
    const uint4 *qdesc;
    const int32_t *cbeg, *cend, *cidx;
    SivoSearchRule rule;
    const uint8_t *blocked;
    const int32_t *owner_prev;   // min blocking accepted query that picked k in the previous round (INT_MAX none); null in round 0
    int32_t *owner_next;
    int32_t *npick;              // accepted picks per keypoint this round
    int32_t *pick, *bdist, *sdist;   // per query: accepted keypoint or -1, best / second distance
    int32_t *flags;              // [0] collision (two accepted picks of one keypoint), [1] a pick changed
};

// top-2 of a (key, index) multiset; key = match_key of the distance and the visiting order (or its complement when the last candidate wins)
struct Top2 { uint32_t k1, k2; int i1, i2; };
__device__ __forceinline__ void top2_push(Top2 &t, uint32_t k, int i) {
    if (k < t.k1) { t.k2 = t.k1; t.i2 = t.i1; t.k1 = k; t.i1 = i; }
    else if (k < t.k2) { t.k2 = k; t.i2 = i; }
}

__global__ __launch_bounds__(256) void search_round_kernel(SearchArgs a) {
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= a.nq) return;
    const SivoSearchQuery Q = a.q[qi];
    Top2 t{KEY_NONE, KEY_NONE, -1, -1};
    if (Q.flags & SIVO_Q_VALID) {
        const uint4 q0 = a.qdesc[(int64_t)qi * 2], q1 = a.qdesc[(int64_t)qi * 2 + 1];
        const int gate = a.rule.gate_mode;
        const MframeView &V = a.V;
        // one candidate (lane-local): static gates, dynamic exclusion, distance
        auto visit = [&](int idx, uint32_t ord) {
            if (a.blocked && a.blocked[idx]) return;
            if (a.owner_prev && a.owner_prev[idx] < qi) return;
            const int lvl = V.oct[idx];
            if (lvl < Q.lvl_lo || lvl > Q.lvl_hi) return;
            const float kx = V.x[idx], ky = V.y[idx];
            if (!a.cidx && !in_window(kx, ky, Q.u, Q.v, Q.radius)) return;
            const float kur = V.ur ? V.ur[idx] : -1.0f;
            if (gate == 1) {
                if (kur > 0) {
                    const float er = fabsf(Q.ur - kur);
                    if (er > Q.gate) return;
                }
            } else if (gate == 2) {
                if (!fuse_chi2_gate(Q.u - kx, Q.v - ky, kur >= 0, Q.ur - kur, V.inv_sigma2[lvl])) return;      // Fuse
            }
            const int d = ham256(q0, q1, V.desc[(int64_t)idx * 2], V.desc[(int64_t)idx * 2 + 1]);
            if (gate == 3) {
                // SearchForTriangulation (ORBmatcher.cc:703-719)
                if (d > a.rule.th_dist) return;
                const bool st1 = (Q.flags & SIVO_Q_STEREO) != 0, st2 = kur >= 0;
                if (!st1 && !st2) {
                    const float distex = a.rule.ex - kx, distey = a.rule.ey - ky;
                    if (distex * distex + distey * distey < 100 * V.scale[lvl]) return;
                }
                const float *F = a.rule.F12;
                const float ea = Q.u * F[0] + Q.v * F[3] + F[6];
                const float eb = Q.u * F[1] + Q.v * F[4] + F[7];
                const float ec = Q.u * F[2] + Q.v * F[5] + F[8];
                const float num = ea * kx + eb * ky + ec;
                const float den = ea * ea + eb * eb;
                if (den == 0) return;
                const float dsqr = num * num / den;
                if (!((double)dsqr < 3.84 * (double)V.sigma2[lvl])) return;
            }
            if (d >= 256) return;                        // bestDist starts at 256 and the test is `dist < bestDist`
            const uint32_t o = a.rule.tie_last ? (0x3fffffu - ord) : ord;
            top2_push(t, match_key(d, o), idx);
        };
        if (a.cidx) {
            const int s = a.cbeg[qi], e = a.cend[qi];
            for (int j = s + lane; j < e; j += 64) visit(a.cidx[j], (uint32_t)(j - s));
        } else {
            scan_window(V, Q.u, Q.v, Q.radius, lane, visit);
        }
    }
    // butterfly: merge the lanes' top-2 sets
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t ok1 = __shfl_xor(t.k1, off), ok2 = __shfl_xor(t.k2, off);
        const int oi1 = __shfl_xor(t.i1, off), oi2 = __shfl_xor(t.i2, off);
        top2_push(t, ok1, oi1);
        top2_push(t, ok2, oi2);
    }
    if (lane != 0) return;
    const int best = t.i1 >= 0 ? (int)(t.k1 >> 22) : 256, second = t.i2 >= 0 ? (int)(t.k2 >> 22) : 256;
    bool accept = t.i1 >= 0 && (a.rule.accept_lt ? best < a.rule.th_dist : best <= a.rule.th_dist);
    if (accept && a.rule.ratio_mode == 1) {
        const int bestLevel = a.V.oct[t.i1], bestLevel2 = t.i2 >= 0 ? a.V.oct[t.i2] : -1;
        if (bestLevel == bestLevel2 && (float)best > a.rule.nn_ratio * (float)second) accept = false;
    } else if (accept && a.rule.ratio_mode == 2) {
        if (!((float)best < a.rule.nn_ratio * (float)second)) accept = false;
    }
    const int p = accept ? t.i1 : -1;
    if (a.pick[qi] != p) a.flags[1] = 1;
    a.pick[qi] = p;
    a.bdist[qi] = best;
    a.sdist[qi] = second;
    if (p >= 0 && a.rule.dynamic) {
        if (atomicAdd(&a.npick[p], 1) > 0) a.flags[0] = 1;
        if (Q.flags & SIVO_Q_BLOCKS) atomicMin(&a.owner_next[p], qi);
    }
}

struct FinalArgs {
    int n, nq;
    const SivoSearchQuery *q;
    const float *angle;
    const int32_t *pick;
    int check_orientation;
    int32_t *match_query, *match_train;   // device outputs (nq / n)
    int32_t *counters;                    // [0] accepted, [1] culled by the rotation check
};

// One workgroup: rotation histogram (ORBmatcher.cc:1376-1412), three maxima (:1545-1577), final slot owners.
__global__ __launch_bounds__(1024) void search_finalize_kernel(FinalArgs a) {
    __shared__ int hist[SIVO_HISTO];
    __shared__ int keep[SIVO_HISTO];
    const int tid = threadIdx.x;
    if (tid < SIVO_HISTO) { hist[tid] = 0; keep[tid] = 1; }
    if (tid < 2) a.counters[tid] = 0;
    for (int k = tid; k < a.n; k += 1024) a.match_train[k] = -1;
    __syncthreads();
    const float factor = 1.0f / SIVO_HISTO;
    int accepted = 0;
    for (int qi = tid; qi < a.nq; qi += 1024) {
        const int p = a.pick[qi];
        if (p < 0) continue;
        ++accepted;
        if (a.check_orientation) {
            float rot = a.q[qi].angle - a.angle[p];
            if (rot < 0.0f) rot += 360.0f;
            int bin = (int)roundf(rot * factor);
            if (bin == SIVO_HISTO) bin = 0;
            atomicAdd(&hist[bin], 1);
        }
    }
    if (accepted) atomicAdd(&a.counters[0], accepted);
    __syncthreads();
    if (tid == 0 && a.check_orientation) {
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < SIVO_HISTO; ++i) {
            const int s = hist[i];
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
            else if (s > max3) { max3 = s; ind3 = i; }
        }
        if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
        for (int i = 0; i < SIVO_HISTO; ++i) keep[i] = (i == ind1 || i == ind2 || i == ind3);
    }
    __syncthreads();
    // slot owners: the blocking picker if there is one (no later query can take the slot), else the last non-blocking one
    for (int qi = tid; qi < a.nq; qi += 1024) {
        const int p = a.pick[qi];
        if (p >= 0 && !(a.q[qi].flags & SIVO_Q_BLOCKS)) atomicMax(&a.match_train[p], qi);
    }
    __syncthreads();
    for (int qi = tid; qi < a.nq; qi += 1024) {
        const int p = a.pick[qi];
        if (p >= 0 && (a.q[qi].flags & SIVO_Q_BLOCKS)) a.match_train[p] = qi;
    }
    __syncthreads();
    int culled = 0;
    for (int qi = tid; qi < a.nq; qi += 1024) {
        const int p = a.pick[qi];
        int m = p;
        if (p >= 0 && a.check_orientation) {
            float rot = a.q[qi].angle - a.angle[p];
            if (rot < 0.0f) rot += 360.0f;
            int bin = (int)roundf(rot * factor);
            if (bin == SIVO_HISTO) bin = 0;
            if (!keep[bin]) { m = -1; ++culled; a.match_train[p] = -2; }
        }
        a.match_query[qi] = m;
    }
    if (culled) atomicAdd(&a.counters[1], culled);
}

// ---- slab pool ------------------------------------------------------------------------------------------------------
struct SlabPool {
    std::mutex mu;
    std::vector<std::unique_ptr<MframeSlab>> idle;
    static constexpr size_t KEEP = 64;          // a local map's keyframes + the tracking frames; beyond that slabs are freed
    std::unique_ptr<MframeSlab> take(int device, size_t bytes) {
        {
            std::lock_guard<std::mutex> lock(mu);
            int best = -1;
            for (size_t i = 0; i < idle.size(); ++i)
                if (idle[i]->device == device && idle[i]->cap >= bytes && (best < 0 || idle[i]->cap < idle[(size_t)best]->cap)) best = (int)i;
            if (best >= 0) {
                std::unique_ptr<MframeSlab> r = std::move(idle[(size_t)best]);
                idle.erase(idle.begin() + best);
                return r;
            }
        }
        std::unique_ptr<MframeSlab> r(new MframeSlab);
        r->device = device;
        r->cap = std::max(bytes, (size_t)1 << 20);
        SIVO_HIP(hipMalloc((void **)&r->d, r->cap));
        SIVO_HIP(hipHostMalloc((void **)&r->h, r->cap, hipHostMallocDefault));
        SIVO_HIP(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
        return r;
    }
    void give(std::unique_ptr<MframeSlab> sl) {
        if (!sl) return;
        (void)hipStreamSynchronize(sl->stream);      // (an upload nobody searched against may still be in flight)
        std::lock_guard<std::mutex> lock(mu);
        if (idle.size() < KEEP) idle.push_back(std::move(sl));
    }
};
SlabPool &slab_pool() {
    static SlabPool *p = new SlabPool;           // never destroyed: frames may be released after main() returns
    return *p;
}

// The frame's arrays at the head of a slab: place() on (slab->d, slab->h) binds F's device pointers, bytes() is F.frame_bytes.
Layout frame_layout(sivo_mframe &F) {
    Layout L;
    const size_t n = (size_t)F.n, lv = 4 * (size_t)F.nlevels;
    L.copy(F.d_x, nullptr, 4 * n); L.copy(F.d_y, nullptr, 4 * n); L.copy(F.d_angle, nullptr, 4 * n); L.copy(F.d_oct, nullptr, 4 * n);
    L.copy(F.d_ur, nullptr, 4 * F.u_right.size());
    L.copy(F.d_desc, nullptr, 32 * n);
    L.copy(F.d_cell_off, nullptr, 4 * F.cell_off.size()); L.copy(F.d_cell_idx, nullptr, 4 * F.cell_idx.size());
    L.copy(F.d_scale, nullptr, lv); L.copy(F.d_sigma2, nullptr, lv); L.copy(F.d_inv_sigma2, nullptr, lv);
    return L;
}

// The engine's scratch behind the frame's arrays; a call that needs more than the slab holds moves the frame to a bigger slab
// (the pinned mirror still holds the frame's arrays: one copy host to host, one upload).
char *scratch(sivo_mframe &F, size_t bytes) {
    if (F.frame_bytes + bytes > F.slab->cap) {
        std::unique_ptr<MframeSlab> big = slab_pool().take(F.device, (F.frame_bytes + bytes) * 2);
        SIVO_HIP(hipStreamSynchronize(F.slab->stream));
        std::memcpy(big->h, F.slab->h, F.frame_bytes);
        SIVO_HIP(hipMemcpyAsync(big->d, big->h, F.frame_bytes, hipMemcpyHostToDevice, big->stream));
        slab_pool().give(std::move(F.slab));
        F.slab = std::move(big);
        F.stream = F.slab->stream;
        frame_layout(F).place(F.slab->d, F.slab->h);
    }
    return F.slab->d + F.frame_bytes;
}

// (DeviceQueries, the interface of a producer that makes the queries on the device, is search_engine.hpp)
struct EngineIn {                // the host arrays of a call (all null where only the size of the layout is asked for)
    const SivoSearchQuery *q;
    const uint8_t *qdesc;
    const int32_t *cbeg, *cend, *cidx;
    const uint8_t *blocked;
};
struct EngineBufs {              // what the layout hands out beside the pointers that live in SearchArgs
    SivoSearchQuery *q;
    int32_t *owner[2];           // [1]: device only
    int32_t *counters, *match_query, *match_train;
    size_t down;                 // the results to copy back, from `counters` on
};

// The engine's regions of one call, the only statement of its scratch: [ upload | results | device-only ].  The upload holds the
// queries, their descriptors, the candidate lists (`lists`), the blocked flags and the regions that START with a value the caller
// writes through L.host() — pick, flags and, for a dynamic rule, owner[0] and npick; the results hold the producer's as well.
// A producer with device_inputs() writes the queries, their descriptors and the blocked flags on the device: they move behind the
// results, and the candidate ranges (read with lists only) take no room.
void engine_layout(Layout &L, SearchArgs &a, EngineBufs &b, int n, int nq, int n_cand, bool dynamic, bool lists, DeviceQueries *dq,
                   const EngineIn &in = EngineIn{}) {
    const size_t N = (size_t)n, Q = (size_t)nq;
    const bool on_device = dq && dq->device_inputs() && !lists;
    if (!on_device) {
        L.copy(b.q, in.q, Q * sizeof(SivoSearchQuery));             // (with dq: written by its kernel)
        L.copy(a.qdesc, in.qdesc, 32 * Q);
        L.copy(a.cbeg, in.cbeg, 4 * Q); L.copy(a.cend, in.cend, 4 * Q); // (read with lists only; their room is part of a call's size)
        if (lists) L.copy(a.cidx, in.cidx, 4 * (size_t)n_cand);
        L.copy(a.blocked, in.blocked, N);
    }
    L.copy(a.pick, nullptr, 4 * Q);                                 // -1
    if (dynamic) { L.copy(b.owner[0], nullptr, 4 * N); L.copy(a.npick, nullptr, 4 * N); }      // 0x7f7f7f7f > any query index; 0
    L.copy(a.flags, nullptr, 16);                                   // collision, changed: 0
    L.take(b.counters, 16);                                         // accepted, culled
    L.take(b.match_query, 4 * Q); L.take(b.match_train, 4 * N); L.take(a.bdist, 4 * Q); L.take(a.sdist, 4 * Q);
    if (dq) dq->regions(L);
    b.down = L.results();
    if (dynamic) L.take(b.owner[1], 4 * N);                         // scratch behind the results: not copied back
    if (on_device) { L.take(b.q, Q * sizeof(SivoSearchQuery)); L.take(a.qdesc, 32 * Q); L.take(a.blocked, N); }
}

}  // namespace

// The engine on host arrays: upload queries, rounds, finalize, download.  With `dq` the queries come from the device and `queries` is
// not read; without it nothing of the layout or the launches changes.  (declared in search_engine.hpp)
void run_search(sivo_mframe &F, const SivoSearchQuery *queries, const uint8_t *query_desc, int nq, const int32_t *cand_begin,
                const int32_t *cand_end, const int32_t *cand_idx, int n_cand, const SivoSearchRule &rule, const uint8_t *blocked,
                int32_t *match_query, int32_t *match_train, int32_t *best_dist, int32_t *second_dist, int *n_matches,
                int *rounds_out, DeviceQueries *dq) {
    if (rounds_out) *rounds_out = 0;
    if (n_matches) *n_matches = 0;
    if (match_train) for (int k = 0; k < F.n; ++k) match_train[k] = -1;
    if (nq <= 0) return;
    if (nq >= (1 << 22) || F.n >= (1 << 22) || n_cand >= (1 << 22)) throw std::invalid_argument("sivo_search: at most 2^22 - 1 queries / keypoints / list entries");
    // explicit candidate lists index the frame's keypoints: a stale or foreign FeatureVector entry would be an out-of-bounds
    // read of descriptors / keys and, through the pick, an out-of-bounds atomic on the scratch buffer
    if (cand_idx)
        for (int j = 0; j < n_cand; ++j)
            if ((uint32_t)cand_idx[j] >= (uint32_t)F.n) throw std::invalid_argument("sivo_search: candidate index outside the frame's keypoints");
    DeviceGuard dg(F.device);
    const int n = F.n;
    // ONE copy up (the layout's copy regions, the initial values among them), one copy down (its take regions but the last)
    SearchArgs a{};
    EngineBufs b{};
    Layout L;
    engine_layout(L, a, b, n, nq, n_cand, rule.dynamic != 0, cand_idx != nullptr, dq,
                  EngineIn{queries, query_desc, cand_begin, cand_end, cand_idx, blocked});
    char *const d0 = scratch(F, L.bytes());
    hipStream_t st = F.stream;
    SIVO_HIP(hipStreamSynchronize(st));          // (the mirror may still feed the frame's own upload)
    L.place(d0, F.slab->h + F.frame_bytes);
    std::memset(L.host(a.pick), 0xff, (size_t)nq * 4);
    if (rule.dynamic) {
        std::memset(L.host(b.owner[0]), 0x7f, (size_t)n * 4);
        std::memset(L.host(a.npick), 0, (size_t)n * 4);
    }
    std::memset(L.host(a.flags), 0, 16);
    L.send(st);
    if (dq) dq->launch(F, EngineRegions{b.q, const_cast<uint4 *>(a.qdesc), const_cast<uint8_t *>(a.blocked)});

    a.V = F.view();
    a.nq = nq; a.q = b.q; a.rule = rule;
    if (!blocked && !(dq && dq->device_inputs())) a.blocked = nullptr;
    int rounds = 0;
    for (;; ++rounds) {
        a.owner_prev = rounds == 0 ? nullptr : b.owner[(rounds + 1) & 1];
        a.owner_next = b.owner[rounds & 1];
        if (rounds && rule.dynamic && n) {                                         // (round 0's values came with the upload)
            SIVO_HIP(hipMemsetAsync(a.owner_next, 0x7f, (size_t)n * 4, st));
            SIVO_HIP(hipMemsetAsync(a.npick, 0, (size_t)n * 4, st));
        }
        if (rounds) SIVO_HIP(hipMemsetAsync(a.flags, 0, 8, st));
        hipLaunchKernelGGL(search_round_kernel, dim3((unsigned)cdiv(nq, 4)), dim3(256), 0, st, a);
        if (!rule.dynamic) { ++rounds; break; }
        int32_t *fl = L.host(a.flags);
        SIVO_HIP(hipMemcpyAsync(fl, a.flags, 8, hipMemcpyDeviceToHost, st));
        SIVO_HIP(hipStreamSynchronize(st));
        // round 0 is final when no keypoint was picked twice — unless a ratio test is on: a keypoint an earlier query took
        // may have been this query's SECOND best, so a confirming round always runs then
        if (rounds == 0 ? (!fl[0] && rule.ratio_mode == 0) : !fl[1]) { ++rounds; break; }
        if (rounds > nq + 1) throw std::runtime_error("sivo_search: the repair rounds did not converge");
    }
    FinalArgs f{};
    f.n = n; f.nq = nq; f.q = b.q; f.angle = a.V.angle; f.pick = a.pick; f.check_orientation = rule.check_orientation;
    f.match_query = b.match_query; f.match_train = b.match_train; f.counters = b.counters;
    hipLaunchKernelGGL(search_finalize_kernel, dim3(1), dim3(1024), 0, st, f);
    SIVO_HIP(hipMemcpyAsync(L.host(b.counters), b.counters, b.down, hipMemcpyDeviceToHost, st));
    SIVO_HIP(hipStreamSynchronize(st));
    SIVO_HIP(hipGetLastError());
    const int32_t *cnt = L.host(b.counters);
    if (match_query) std::memcpy(match_query, L.host(b.match_query), (size_t)nq * 4);
    if (match_train && n) std::memcpy(match_train, L.host(b.match_train), (size_t)n * 4);
    if (best_dist) std::memcpy(best_dist, L.host(a.bdist), (size_t)nq * 4);
    if (second_dist) std::memcpy(second_dist, L.host(a.sdist), (size_t)nq * 4);
    if (n_matches) *n_matches = cnt[0] - cnt[1];
    if (rounds_out) *rounds_out = rounds;
    if (dq) dq->collect(L);
}

namespace {

// Frame::GetFeaturesInArea (Frame.cc:326-390) on the host copy of the grid.
void features_in_area(const sivo_mframe &F, float x, float y, float r, int minLevel, int maxLevel, std::vector<int32_t> &out) {
    out.clear();
    int nMinCellX, nMaxCellX, nMinCellY, nMaxCellY;
    if (!grid_window(F.min_x, F.min_y, F.inv_w, F.inv_h, x, y, r, nMinCellX, nMaxCellX, nMinCellY, nMaxCellY)) return;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
        for (int iy = nMinCellY; iy <= nMaxCellY; iy++)
            for (int j = F.cell_off[ix * SIVO_GRID_ROWS + iy]; j < F.cell_off[ix * SIVO_GRID_ROWS + iy + 1]; ++j) {
                const SivoKeyPoint &kp = F.keys[F.cell_idx[j]];
                if (bCheckLevels) {
                    if (kp.octave < minLevel) continue;
                    if (maxLevel >= 0 && kp.octave > maxLevel) continue;
                }
                if (in_window(kp.x, kp.y, x, y, r)) out.push_back(F.cell_idx[j]);
            }
}

// GetFeaturesInArea(min, max) tests `octave < min` only when (min > 0 || max >= 0) and `octave > max` only when
// max >= 0; with octave >= 0 that is the plain range [min, max >= 0 ? max : inf).
void level_range(int minLevel, int maxLevel, int32_t &lo, int32_t &hi) {
    lo = minLevel;
    hi = maxLevel >= 0 ? maxLevel : INT_MAX;
}

}  // namespace

SivoSearchRule make_rule(int th, int gate_mode, int ratio_mode, float nn, bool ori, bool dynamic) {
    SivoSearchRule r;
    std::memset(&r, 0, sizeof r);
    r.th_dist = th; r.gate_mode = gate_mode; r.ratio_mode = ratio_mode; r.nn_ratio = nn;
    r.check_orientation = ori ? 1 : 0; r.dynamic = dynamic ? 1 : 0;
    return r;
}

namespace {

void require(bool ok, const char *what) {
    if (!ok) throw std::invalid_argument(what);
}

// ---- Tracking::SearchLocalPoints: the cull and the queries of the points in view, on the device --------------------------------
// One thread per map point: Frame::isInFrustum (frustum_math.hpp, the function frustum.hip runs), then the query record exactly as
// sivo_search_by_projection_mappoints builds it on the host, written straight into the engine's query block; a point that is not in
// view leaves a zeroed record (flags 0: the round kernel skips it).
struct FrQueryArgs {
    FrCamera cam;
    int n;
    float th;
    const float *pos, *normal, *min_dist, *max_dist;
    const uint8_t *skip;           // may be null
    const int32_t *obs;
    const float *scale;            // the frame's mvScaleFactors (cam.f.nlevels <= the frame's levels)
    SivoSearchQuery *q;
    uint8_t *status;
    float *px, *py, *pxr, *vc;     // written for the points in view only
    int32_t *level;
};

__global__ __launch_bounds__(256) void fr_queries_kernel(FrQueryArgs a) {
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= a.n) return;
    uint8_t st = SIVO_FRUSTUM_SKIPPED;
    FrResult o;
    if (!(a.skip && a.skip[i])) {
        const float X[3] = {a.pos[3 * (int64_t)i], a.pos[3 * (int64_t)i + 1], a.pos[3 * (int64_t)i + 2]};
        const float N[3] = {a.normal[3 * (int64_t)i], a.normal[3 * (int64_t)i + 1], a.normal[3 * (int64_t)i + 2]};
        st = fr_point(a.cam, X, N, a.min_dist[i], a.max_dist[i], o);
    }
    SivoSearchQuery q;
    if (st == SIVO_FRUSTUM_IN_VIEW) {
        fr_query(o, a.th, a.scale, a.obs[i], q);
        a.px[i] = o.u; a.py[i] = o.v; a.pxr[i] = o.ur; a.vc[i] = o.view_cos; a.level[i] = o.level;
    } else {
        fr_no_query(q);
    }
    a.q[i] = q;
    a.status[i] = st;
}

struct LocalPointQueries : DeviceQueries {
    FrQueryArgs a;
    size_t N;
    const float *pos, *normal, *min_dist, *max_dist;      // the caller's host arrays
    const uint8_t *skip;
    const int32_t *obs;
    uint8_t *status;
    float *px, *py, *pxr, *vc;                             // each may be null
    int32_t *level;
    int n_to_match = 0;
    explicit LocalPointQueries(size_t n) : N(n) {}
    void regions(Layout &L) override {
        L.copy(a.pos, pos, 12 * N); L.copy(a.normal, normal, 12 * N); L.copy(a.min_dist, min_dist, 4 * N); L.copy(a.max_dist, max_dist, 4 * N);
        L.copy(a.obs, obs, 4 * N);
        a.skip = nullptr;
        if (skip) L.copy(a.skip, skip, N);
        L.take(a.status, N); L.take(a.px, 4 * N); L.take(a.py, 4 * N); L.take(a.pxr, 4 * N); L.take(a.vc, 4 * N); L.take(a.level, 4 * N);
    }
    void launch(const sivo_mframe &F, const EngineRegions &r) override {
        a.scale = F.view().scale;                                  // (after scratch(): the frame may have moved to a bigger slab)
        a.q = r.q;
        hipLaunchKernelGGL(fr_queries_kernel, dim3((unsigned)cdiv((int)N, 256)), dim3(256), 0, F.stream, a);
        SIVO_HIP(hipGetLastError());
    }
    void collect(const Layout &L) override {
        const uint8_t *hs = L.host(a.status);
        const float *hx = L.host(a.px), *hy = L.host(a.py), *hr = L.host(a.pxr), *hc = L.host(a.vc);
        const int32_t *hl = L.host(a.level);
        for (size_t i = 0; i < N; ++i) {
            status[i] = hs[i];
            if (hs[i] != SIVO_FRUSTUM_IN_VIEW) continue;               // nothing else of the point is written
            ++n_to_match;
            if (px) px[i] = hx[i];
            if (py) py[i] = hy[i];
            if (pxr) pxr[i] = hr[i];
            if (vc) vc[i] = hc[i];
            if (level) level[i] = hl[i];
        }
    }
};

}  // namespace
}  // namespace sivo

using namespace sivo;

sivo_mframe::~sivo_mframe() { slab_pool().give(std::move(slab)); }

extern "C" int sivo_mframe_create(const SivoKeyPoint *keys, int n, const float *u_right, const uint8_t *descriptors,
                                  float min_x, float max_x, float min_y, float max_y, const float *scale_factors,
                                  const float *level_sigma2, const float *inv_level_sigma2, int nlevels, int device,
                                  sivo_mframe_t *out) {
    return guarded([&] {
        require(out != nullptr, "out is NULL");
        *out = nullptr;
        require(n >= 0 && (n == 0 || (keys && descriptors)), "keys / descriptors are NULL");
        require(nlevels > 0 && scale_factors && level_sigma2 && inv_level_sigma2, "scale tables are NULL");
        require(max_x > min_x && max_y > min_y, "empty image bounds");
        require_device();
        if (device < 0) SIVO_HIP(hipGetDevice(&device));                    // -1: the calling thread's current device
        if (sivo_device_count() <= device)
            return fail(SIVO_ERR_RUNTIME, "HIP device %d is not available (%d visible): libsivo_hip has no CPU fallback", device,
                        sivo_device_count());
        std::unique_ptr<sivo_mframe> F(new sivo_mframe);
        F->device = device; F->n = n; F->nlevels = nlevels;
        F->min_x = min_x; F->max_x = max_x; F->min_y = min_y; F->max_y = max_y;
        F->inv_w = (float)SIVO_GRID_COLS / (max_x - min_x);
        F->inv_h = (float)SIVO_GRID_ROWS / (max_y - min_y);
        F->keys.assign(keys, keys + n);
        if (u_right) F->u_right.assign(u_right, u_right + n);
        F->scale.assign(scale_factors, scale_factors + nlevels);
        F->sigma2.assign(level_sigma2, level_sigma2 + nlevels);
        F->inv_sigma2.assign(inv_level_sigma2, inv_level_sigma2 + nlevels);
        for (int i = 0; i < n; ++i) require(keys[i].octave >= 0 && keys[i].octave < nlevels, "keypoint octave outside the scale tables");
        grid_build(keys, n, min_x, min_y, F->inv_w, F->inv_h, F->cell_off, F->cell_idx);

        DeviceGuard dg(device);
        // one slab: the frame's arrays + the engine's scratch for a dynamic call with candidate lists and as many queries as the
        // frame has keys (a bigger call grows it)
        Layout L = frame_layout(*F), guess;
        SearchArgs ga{};
        EngineBufs gb{};
        engine_layout(guess, ga, gb, n, n, 0, true, true, nullptr);
        F->frame_bytes = L.bytes();
        F->slab = slab_pool().take(device, F->frame_bytes + guess.bytes());
        F->stream = F->slab->stream;
        L.place(F->slab->d, F->slab->h);
        float *hx = L.host(F->d_x), *hy = L.host(F->d_y), *ha = L.host(F->d_angle);
        int32_t *ho = L.host(F->d_oct);
        for (int i = 0; i < n; ++i) { hx[i] = keys[i].x; hy[i] = keys[i].y; ha[i] = keys[i].angle; ho[i] = keys[i].octave; }
        if (!F->u_right.empty()) std::memcpy(L.host(F->d_ur), F->u_right.data(), F->u_right.size() * 4);
        if (n) std::memcpy(L.host(F->d_desc), descriptors, (size_t)n * 32);
        std::memcpy(L.host(F->d_cell_off), F->cell_off.data(), F->cell_off.size() * 4);
        if (!F->cell_idx.empty()) std::memcpy(L.host(F->d_cell_idx), F->cell_idx.data(), F->cell_idx.size() * 4);
        std::memcpy(L.host(F->d_scale), F->scale.data(), (size_t)nlevels * 4);
        std::memcpy(L.host(F->d_sigma2), F->sigma2.data(), (size_t)nlevels * 4);
        std::memcpy(L.host(F->d_inv_sigma2), F->inv_sigma2.data(), (size_t)nlevels * 4);
        // (asynchronous: every search of this frame runs on the same stream, behind the upload)
        L.send(F->stream);
        *out = F.release();
        return SIVO_OK;
    });
}

extern "C" int sivo_mframe_destroy(sivo_mframe_t h) {
    return guarded([&] {
        if (h) {
            DeviceGuard dg(h->device);
            delete h;
        }
        return SIVO_OK;
    });
}

extern "C" int sivo_mframe_slab_bytes(sivo_mframe_t h, int64_t *bytes) {
    return guarded([&] {
        require(h && bytes, "null argument");
        *bytes = (int64_t)h->slab->cap;
        return SIVO_OK;
    });
}

extern "C" int sivo_mframe_features_in_area(sivo_mframe_t h, float x, float y, float r, int min_level, int max_level,
                                            int32_t *out, int capacity, int *n_out) {
    return guarded([&] {
        require(h && n_out, "null argument");
        std::vector<int32_t> v;
        features_in_area(*h, x, y, r, min_level, max_level, v);
        *n_out = (int)v.size();
        if (!out) return SIVO_OK;
        if (capacity < (int)v.size()) return fail(SIVO_ERR_CAPACITY, "%zu indices, capacity %d", v.size(), capacity);
        std::memcpy(out, v.data(), v.size() * 4);
        return SIVO_OK;
    });
}

extern "C" int sivo_search(sivo_mframe_t train, const SivoSearchQuery *queries, const uint8_t *query_desc, int n_queries,
                           const int32_t *cand_begin, const int32_t *cand_end, const int32_t *cand_idx, int n_cand,
                           const SivoSearchRule *rule, const uint8_t *blocked, int32_t *match_query, int32_t *match_train,
                           int32_t *best_dist, int32_t *second_dist, int *n_matches, int *rounds) {
    return guarded([&] {
        require(train && rule && n_queries >= 0 && (n_queries == 0 || (queries && query_desc)), "null argument");
        require(!cand_idx || (cand_begin && cand_end), "explicit candidate lists need cand_begin and cand_end");
        if (cand_idx)
            for (int q = 0; q < n_queries; ++q)
                require(cand_begin[q] >= 0 && cand_begin[q] <= cand_end[q] && cand_end[q] <= n_cand, "candidate range outside the list");
        run_search(*train, queries, query_desc, n_queries, cand_begin, cand_end, cand_idx, n_cand, *rule, blocked, match_query,
                   match_train, best_dist, second_dist, n_matches, rounds);
        return SIVO_OK;
    });
}

// ---- the reference routines on arrays -------------------------------------------------------------------------------

extern "C" int sivo_search_by_projection_mappoints(sivo_mframe_t F, int n_mp, const uint8_t *track_in_view, const float *proj_x,
                                                   const float *proj_y, const float *proj_xr, const int32_t *level,
                                                   const float *view_cos, const uint8_t *mp_desc, const int32_t *mp_obs,
                                                   float th, float nn_ratio, int32_t *occ_obs, int32_t *match, int *n_matches) {
    return guarded([&] {
        require(F && n_mp >= 0 && occ_obs && match, "null argument");
        require(n_mp == 0 || (track_in_view && proj_x && proj_y && proj_xr && level && view_cos && mp_desc && mp_obs), "null argument");
        const bool bFactor = th != 1.0;
        std::vector<SivoSearchQuery> q((size_t)n_mp);
        for (int i = 0; i < n_mp; ++i) {
            SivoSearchQuery &s = q[i];
            std::memset(&s, 0, sizeof s);
            if (!track_in_view[i]) continue;
            require(level[i] >= 0 && level[i] < F->nlevels, "predicted level outside the scale tables");
            float r = view_cos[i] > 0.998 ? 2.5f : 4.0f;                    // RadiusByViewingCos (ORBmatcher.cc:129-134)
            if (bFactor) r *= th;
            s.u = proj_x[i]; s.v = proj_y[i];
            s.radius = r * F->scale[level[i]];
            level_range(level[i] - 1, level[i], s.lvl_lo, s.lvl_hi);
            s.ur = proj_xr[i]; s.gate = r * F->scale[level[i]];
            s.flags = SIVO_Q_VALID | (mp_obs[i] > 0 ? SIVO_Q_BLOCKS : 0);
        }
        std::vector<uint8_t> blocked((size_t)F->n);
        for (int k = 0; k < F->n; ++k) blocked[k] = occ_obs[k] > 0;
        const SivoSearchRule rule = make_rule(SIVO_TH_HIGH, 1, 1, nn_ratio, false, true);
        run_search(*F, q.data(), mp_desc, n_mp, nullptr, nullptr, nullptr, 0, rule, blocked.data(), nullptr, match, nullptr, nullptr,
                   n_matches, nullptr);
        for (int k = 0; k < F->n; ++k)
            if (match[k] >= 0) occ_obs[k] = mp_obs[match[k]];
        return SIVO_OK;
    });
}

extern "C" int sivo_search_local_points(sivo_mframe_t F, const SivoFrustum *frustum, int n, const float *pos, const float *normal,
                                        const float *min_dist, const float *max_dist, const uint8_t *skip, const uint8_t *mp_desc,
                                        const int32_t *mp_obs, float th, float nn_ratio, int32_t *occ_obs, int32_t *match,
                                        uint8_t *status, float *proj_x, float *proj_y, float *proj_xr, float *view_cos,
                                        int32_t *level, int *n_to_match, int *n_matches) {
    return guarded([&] {
        require(F && frustum && n >= 0 && occ_obs && match, "null argument");
        require(n == 0 || (pos && normal && min_dist && max_dist && mp_desc && mp_obs && status), "null argument");
        require(frustum->nlevels >= 1 && frustum->nlevels <= 16, "nlevels outside 1 .. 16");
        require(frustum->nlevels <= F->nlevels, "the frustum has more levels than the frame's scale tables");
        LocalPointQueries lp((size_t)n);
        require(fr_camera(*frustum, lp.a.cam), "log_scale_factor must be positive");
        lp.a.n = n; lp.a.th = th; lp.a.scale = nullptr;             // (the frame's scale table: set in launch)
        lp.pos = pos; lp.normal = normal; lp.min_dist = min_dist; lp.max_dist = max_dist; lp.skip = skip; lp.obs = mp_obs;
        lp.status = status; lp.px = proj_x; lp.py = proj_y; lp.pxr = proj_xr; lp.vc = view_cos; lp.level = level;
        std::vector<uint8_t> blocked((size_t)F->n);
        for (int k = 0; k < F->n; ++k) blocked[k] = occ_obs[k] > 0;
        const SivoSearchRule rule = make_rule(SIVO_TH_HIGH, 1, 1, nn_ratio, false, true);
        run_search(*F, nullptr, mp_desc, n, nullptr, nullptr, nullptr, 0, rule, blocked.data(), nullptr, match, nullptr, nullptr, n_matches,
                   nullptr, &lp);
        for (int k = 0; k < F->n; ++k)
            if (match[k] >= 0) occ_obs[k] = mp_obs[match[k]];
        if (n_to_match) *n_to_match = lp.n_to_match;
        return SIVO_OK;
    });
}

extern "C" int sivo_search_by_projection_frame(sivo_mframe_t C, int n_last, const uint8_t *valid, const float *u, const float *v,
                                               const float *inv_z, const int32_t *last_octave, const float *last_angle,
                                               const uint8_t *mp_desc, const int32_t *mp_obs, float th, int forward, int backward,
                                               float bf, int check_orientation, int32_t *occ_obs, int32_t *match,
                                               int *n_matches) {
    return guarded([&] {
        require(C && n_last >= 0 && occ_obs && match, "null argument");
        require(n_last == 0 || (valid && u && v && inv_z && last_octave && last_angle && mp_desc && mp_obs), "null argument");
        std::vector<SivoSearchQuery> q((size_t)n_last);
        for (int i = 0; i < n_last; ++i) {
            SivoSearchQuery &s = q[i];
            std::memset(&s, 0, sizeof s);
            if (!valid[i]) continue;
            if (inv_z[i] < 0) continue;                                                  // :1318-1319
            if (u[i] < C->min_x || u[i] > C->max_x) continue;                            // :1324-1327
            if (v[i] < C->min_y || v[i] > C->max_y) continue;
            const int oct = last_octave[i];
            require(oct >= 0 && oct < C->nlevels, "octave outside the scale tables");
            s.u = u[i]; s.v = v[i];
            s.radius = th * C->scale[oct];
            if (forward) level_range(oct, -1, s.lvl_lo, s.lvl_hi);                       // :1336-1343
            else if (backward) level_range(0, oct, s.lvl_lo, s.lvl_hi);
            else level_range(oct - 1, oct + 1, s.lvl_lo, s.lvl_hi);
            s.ur = u[i] - bf * inv_z[i];                                                 // :1354
            s.gate = s.radius;
            s.angle = last_angle[i];
            s.flags = SIVO_Q_VALID | (mp_obs[i] > 0 ? SIVO_Q_BLOCKS : 0);
        }
        std::vector<uint8_t> blocked((size_t)C->n);
        for (int k = 0; k < C->n; ++k) blocked[k] = occ_obs[k] > 0;
        const SivoSearchRule rule = make_rule(SIVO_TH_HIGH, 1, 0, 0.f, check_orientation != 0, true);
        run_search(*C, q.data(), mp_desc, n_last, nullptr, nullptr, nullptr, 0, rule, blocked.data(), nullptr, match, nullptr, nullptr,
                   n_matches, nullptr);
        for (int k = 0; k < C->n; ++k) {
            if (match[k] >= 0) occ_obs[k] = mp_obs[match[k]];
            else if (match[k] == -2) occ_obs[k] = -1;
        }
        return SIVO_OK;
    });
}

extern "C" int sivo_search_by_projection_reloc(sivo_mframe_t C, int n_kf, const uint8_t *valid, const float *u, const float *v,
                                               const int32_t *pred_level, const float *kf_angle, const uint8_t *mp_desc, float th,
                                               int orb_dist, int check_orientation, uint8_t *occupied, int32_t *match,
                                               int *n_matches) {
    return guarded([&] {
        require(C && n_kf >= 0 && occupied && match, "null argument");
        require(n_kf == 0 || (valid && u && v && pred_level && kf_angle && mp_desc), "null argument");
        // (with ORBdist >= 256 the reference's `bestDist <= ORBdist` holds for a point without any candidate and it indexes
        // mvpMapPoints[-1]; its callers pass 100 and 64, Tracking.cc:1073-1083)
        require(orb_dist >= 0 && orb_dist < 256, "ORBdist must be below 256");
        std::vector<SivoSearchQuery> q((size_t)n_kf);
        for (int i = 0; i < n_kf; ++i) {
            SivoSearchQuery &s = q[i];
            std::memset(&s, 0, sizeof s);
            if (!valid[i]) continue;
            if (u[i] < C->min_x || u[i] > C->max_x) continue;
            if (v[i] < C->min_y || v[i] > C->max_y) continue;
            require(pred_level[i] >= 0 && pred_level[i] < C->nlevels, "predicted level outside the scale tables");
            s.u = u[i]; s.v = v[i];
            s.radius = th * C->scale[pred_level[i]];
            level_range(pred_level[i] - 1, pred_level[i] + 1, s.lvl_lo, s.lvl_hi);
            s.angle = kf_angle[i];
            s.flags = SIVO_Q_VALID | SIVO_Q_BLOCKS;
        }
        const SivoSearchRule rule = make_rule(orb_dist, 0, 0, 0.f, check_orientation != 0, true);
        run_search(*C, q.data(), mp_desc, n_kf, nullptr, nullptr, nullptr, 0, rule, occupied, nullptr, match, nullptr, nullptr, n_matches,
                   nullptr);
        for (int k = 0; k < C->n; ++k) {
            if (match[k] >= 0) occupied[k] = 1;
            else if (match[k] == -2) occupied[k] = 0;
        }
        return SIVO_OK;
    });
}

namespace {
// the shared shape of SearchByProjection(KF, Scw), Fuse x2 and SearchBySim3: window without level arguments, then an
// explicit octave test [pred - 1, pred]
void window_queries(const sivo_mframe &F, int n, const uint8_t *valid, const float *u, const float *v, const float *ur,
                    const int32_t *pred_level, float th, int flags, std::vector<SivoSearchQuery> &q) {
    q.assign((size_t)n, SivoSearchQuery{});
    for (int i = 0; i < n; ++i) {
        SivoSearchQuery &s = q[i];
        std::memset(&s, 0, sizeof s);
        if (!valid[i]) continue;
        require(pred_level[i] >= 0 && pred_level[i] < F.nlevels, "predicted level outside the scale tables");
        s.u = u[i]; s.v = v[i];
        s.radius = th * F.scale[pred_level[i]];
        s.lvl_lo = pred_level[i] - 1; s.lvl_hi = pred_level[i];
        s.ur = ur ? ur[i] : 0.f;
        s.flags = SIVO_Q_VALID | flags;
    }
}
}  // namespace

extern "C" int sivo_search_by_projection_kf(sivo_mframe_t KF, int n_mp, const uint8_t *valid, const float *u, const float *v,
                                            const int32_t *pred_level, const uint8_t *mp_desc, int th, uint8_t *matched,
                                            int32_t *match, int *n_matches) {
    return guarded([&] {
        require(KF && n_mp >= 0 && matched && match, "null argument");
        require(n_mp == 0 || (valid && u && v && pred_level && mp_desc), "null argument");
        std::vector<SivoSearchQuery> q;
        window_queries(*KF, n_mp, valid, u, v, nullptr, pred_level, (float)th, SIVO_Q_BLOCKS, q);
        const SivoSearchRule rule = make_rule(SIVO_TH_LOW, 0, 0, 0.f, false, true);
        run_search(*KF, q.data(), mp_desc, n_mp, nullptr, nullptr, nullptr, 0, rule, matched, nullptr, match, nullptr, nullptr, n_matches,
                   nullptr);
        for (int k = 0; k < KF->n; ++k)
            if (match[k] >= 0) matched[k] = 1;
        return SIVO_OK;
    });
}

extern "C" int sivo_fuse(sivo_mframe_t KF, int n_mp, const uint8_t *valid, const float *u, const float *v, const float *ur,
                         const int32_t *pred_level, const uint8_t *mp_desc, float th, int scw_variant, int32_t *best_idx,
                         int32_t *best_dist, int *n_fused) {
    return guarded([&] {
        require(KF && n_mp >= 0 && best_idx, "null argument");
        require(n_mp == 0 || (valid && u && v && pred_level && mp_desc && (scw_variant || ur)), "null argument");
        std::vector<SivoSearchQuery> q;
        window_queries(*KF, n_mp, valid, u, v, ur, pred_level, th, 0, q);
        const SivoSearchRule rule = make_rule(SIVO_TH_LOW, scw_variant ? 0 : 2, 0, 0.f, false, false);
        std::vector<int32_t> bd((size_t)n_mp);
        run_search(*KF, q.data(), mp_desc, n_mp, nullptr, nullptr, nullptr, 0, rule, nullptr, best_idx, nullptr, bd.data(), nullptr,
                   n_fused, nullptr);
        if (best_dist)      // bestDist starts at 256 (:865) resp. INT_MAX (:1019) and is returned as the loop left it
            for (int i = 0; i < n_mp; ++i) best_dist[i] = (bd[i] == 256 && scw_variant) ? INT_MAX : bd[i];
        return SIVO_OK;
    });
}

extern "C" int sivo_search_by_sim3_dir(sivo_mframe_t KF, int n, const uint8_t *valid, const float *u, const float *v,
                                       const int32_t *pred_level, const uint8_t *mp_desc, float th, int32_t *match_out) {
    return guarded([&] {
        require(KF && n >= 0 && match_out, "null argument");
        require(n == 0 || (valid && u && v && pred_level && mp_desc), "null argument");
        std::vector<SivoSearchQuery> q;
        window_queries(*KF, n, valid, u, v, nullptr, pred_level, th, 0, q);
        const SivoSearchRule rule = make_rule(SIVO_TH_HIGH, 0, 0, 0.f, false, false);
        run_search(*KF, q.data(), mp_desc, n, nullptr, nullptr, nullptr, 0, rule, nullptr, match_out, nullptr, nullptr, nullptr, nullptr,
                   nullptr);
        return SIVO_OK;
    });
}

namespace {
// queries of a BoW-guided routine in the reference's visiting order: node by node, the first operand's keys of the node
struct NodeQueries {
    std::vector<SivoSearchQuery> q;
    std::vector<uint8_t> desc;
    std::vector<int32_t> cbeg, cend, key;      // key[q] = index of the query's keypoint in operand 1
};
template <class ValidFn, class FlagFn>
void node_queries(int n_nodes, const int32_t *off1, const int32_t *idx1, const int32_t *off2, const SivoKeyPoint *keys1,
                  const uint8_t *desc1, int n1, int n2_list, ValidFn valid, FlagFn flags, NodeQueries &out) {
    require(n_nodes >= 0 && (n_nodes == 0 || (off1 && idx1 && off2)), "null node lists");
    for (int k = 0; k < n_nodes; ++k) {
        require(off1[k] <= off1[k + 1] && off2[k] <= off2[k + 1] && off2[k + 1] <= n2_list, "node offsets are not ascending");
        for (int j = off1[k]; j < off1[k + 1]; ++j) {
            const int i1 = idx1[j];
            require(i1 >= 0 && i1 < n1, "node list index outside the first operand");
            SivoSearchQuery s;
            std::memset(&s, 0, sizeof s);
            s.lvl_lo = INT_MIN; s.lvl_hi = INT_MAX;
            s.u = keys1[i1].x; s.v = keys1[i1].y; s.angle = keys1[i1].angle;
            s.flags = valid(i1) ? (SIVO_Q_VALID | flags(i1)) : 0;
            out.q.push_back(s);
            out.desc.insert(out.desc.end(), desc1 + 32 * (size_t)i1, desc1 + 32 * (size_t)i1 + 32);
            out.cbeg.push_back(off2[k]); out.cend.push_back(off2[k + 1]); out.key.push_back(i1);
        }
    }
}
}  // namespace

extern "C" int sivo_search_by_bow_kf_frame(int n_nodes, const int32_t *off1, const int32_t *idx1, const int32_t *off2,
                                           const int32_t *idx2, const uint8_t *kf_valid, const SivoKeyPoint *keys_kf,
                                           const uint8_t *desc_kf, int n_kf, sivo_mframe_t F, float nn_ratio,
                                           int check_orientation, int32_t *match_f, int *n_matches) {
    return guarded([&] {
        require(F && match_f && kf_valid && keys_kf && desc_kf, "null argument");
        const int n2 = n_nodes > 0 ? off2[n_nodes] : 0;
        NodeQueries nq;
        node_queries(n_nodes, off1, idx1, off2, keys_kf, desc_kf, n_kf, n2, [&](int i) { return kf_valid[i] != 0; },
                     [](int) { return SIVO_Q_BLOCKS; }, nq);
        const SivoSearchRule rule = make_rule(SIVO_TH_LOW, 0, 2, nn_ratio, check_orientation != 0, true);
        run_search(*F, nq.q.data(), nq.desc.data(), (int)nq.q.size(), nq.cbeg.data(), nq.cend.data(), idx2, n2, rule, nullptr, nullptr,
                   match_f, nullptr, nullptr, n_matches, nullptr);
        for (int k = 0; k < F->n; ++k) match_f[k] = match_f[k] >= 0 ? nq.key[match_f[k]] : -1;      // :272-275 stores NULL
        return SIVO_OK;
    });
}

extern "C" int sivo_search_by_bow_kf_kf(int n_nodes, const int32_t *off1, const int32_t *idx1, const int32_t *off2,
                                        const int32_t *idx2, const uint8_t *valid1, const SivoKeyPoint *keys1,
                                        const uint8_t *desc1, int n1, const uint8_t *valid2, sivo_mframe_t KF2, float nn_ratio,
                                        int check_orientation, int32_t *matches12, int *n_matches) {
    return guarded([&] {
        require(KF2 && matches12 && valid1 && valid2 && keys1 && desc1 && n1 >= 0, "null argument");
        const int n2 = n_nodes > 0 ? off2[n_nodes] : 0;
        NodeQueries nq;
        node_queries(n_nodes, off1, idx1, off2, keys1, desc1, n1, n2, [&](int i) { return valid1[i] != 0; },
                     [](int) { return SIVO_Q_BLOCKS; }, nq);
        std::vector<uint8_t> blocked((size_t)KF2->n);
        for (int k = 0; k < KF2->n; ++k) blocked[k] = !valid2[k];
        SivoSearchRule rule = make_rule(SIVO_TH_LOW, 0, 2, nn_ratio, check_orientation != 0, true);
        rule.accept_lt = 1;                                                                          // :580 `bestDist1 < TH_LOW`
        std::vector<int32_t> mq(nq.q.size());
        run_search(*KF2, nq.q.data(), nq.desc.data(), (int)nq.q.size(), nq.cbeg.data(), nq.cend.data(), idx2, n2, rule, blocked.data(),
                   mq.data(), nullptr, nullptr, nullptr, n_matches, nullptr);
        for (int i = 0; i < n1; ++i) matches12[i] = -1;
        for (size_t q = 0; q < mq.size(); ++q)
            if (mq[q] >= 0) matches12[nq.key[q]] = mq[q];
        return SIVO_OK;
    });
}

extern "C" int sivo_search_for_triangulation(int n_nodes, const int32_t *off1, const int32_t *idx1, const int32_t *off2,
                                             const int32_t *idx2, const SivoKeyPoint *keys1, const float *u_right1,
                                             const uint8_t *has_mp1, const uint8_t *desc1, int n1, sivo_mframe_t KF2,
                                             const uint8_t *has_mp2, const float F12[9], float ex, float ey, int only_stereo,
                                             int check_orientation, int32_t *matches12, int *n_matches) {
    return guarded([&] {
        require(KF2 && matches12 && keys1 && has_mp1 && has_mp2 && desc1 && F12 && n1 >= 0, "null argument");
        const int n2 = n_nodes > 0 ? off2[n_nodes] : 0;
        NodeQueries nq;
        auto stereo1 = [&](int i) { return u_right1 && u_right1[i] >= 0; };
        node_queries(n_nodes, off1, idx1, off2, keys1, desc1, n1, n2,
                     [&](int i) { return !has_mp1[i] && (!only_stereo || stereo1(i)); },                 // :672-684
                     [&](int i) { return stereo1(i) ? SIVO_Q_STEREO : 0; }, nq);
        std::vector<uint8_t> blocked((size_t)KF2->n);
        for (int k = 0; k < KF2->n; ++k)                                                                  // :694-703 (vbMatched2 is never set)
            blocked[k] = has_mp2[k] || (only_stereo && !(!KF2->u_right.empty() && KF2->u_right[k] >= 0));
        SivoSearchRule rule = make_rule(SIVO_TH_LOW, 3, 0, 0.f, check_orientation != 0, false);
        rule.tie_last = 1;
        std::memcpy(rule.F12, F12, sizeof rule.F12);
        rule.ex = ex; rule.ey = ey;
        std::vector<int32_t> mq(nq.q.size());
        run_search(*KF2, nq.q.data(), nq.desc.data(), (int)nq.q.size(), nq.cbeg.data(), nq.cend.data(), idx2, n2, rule, blocked.data(),
                   mq.data(), nullptr, nullptr, nullptr, n_matches, nullptr);
        for (int i = 0; i < n1; ++i) matches12[i] = -1;
        for (size_t q = 0; q < mq.size(); ++q)
            if (mq[q] >= 0) matches12[nq.key[q]] = mq[q];
        return SIVO_OK;
    });
}
