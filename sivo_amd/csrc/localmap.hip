// localmap.hip — Tracking::UpdateLocalMap (reference src/orbslam/Tracking.cc:1087-1235) on a map that stays on the device: the tables of
// SivoLocalMapTables are uploaded by sivo_localmap_create / _replace, sivo_localmap_set_bad scatters the isBad() flags that change in
// between, and sivo_localmap_update runs one frame: one upload of the frame's lists, five launches, one download, one synchronisation.
// The per-item bodies and the argument checks are localmap_math.hpp; everything is integer and no result depends on the order in which
// atomics arrive (adds, ors, minima and maxima only).
//
// localmap_vote_kernel     ONE workgroup: the counting loop of :1129-1142 (cv_count_slot of covis_math.hpp, self = -1) into a histogram in
//                          LDS, or into the zeroed counts in global memory above SIVO_COVIS_LDS_KF keyframes; writes slot_cleared.
// localmap_select_kernel   ONE workgroup.  Stage 1 (:1156-1172): an order-preserving compaction over kf_order, a ballot per wave and a
//                          prefix over the waves, the first strict maximum carried as one (count, position) key.  Stage 2 (:1177-1229)
//                          is sequential: wave 0 walks the stage-1 keyframes, the ten covisibles on ten lanes, the children in chunks of
//                          64 lanes, a ballot and its lowest set lane give "the first that is not bad and not marked"; every break is
//                          the same in all lanes.  The marks (mnTrackReferenceForFrame == the frame's id) are a bitmap, in LDS up to
//                          SIVO_COVIS_LDS_KF keyframes and in global memory above.  Then the whole workgroup writes the exclusive prefix
//                          of the local keyframes' slot counts (list_off) and stamps the premarked points into first[].
// localmap_first_kernel    pass 1 over the slot sequence g: atomicMin(first[p], g + 1).
// localmap_count_kernel    pass 2a: how many slots of each block of 256 push their point.
// localmap_scatter_kernel  pass 2b: exclusive scan inside the block, the sum of the blocks before it, the scatter in order.
//                          (the bodies of the three point passes, the handle and the workgroup scans are localmap_handle.hpp, which
//                          ba_window.hip shares)
//
// G and the list lengths stay on the device between the launches (hdr); the grids of the three point kernels are sized from a bound the
// host knows: the handle's total slot count (the local list holds no keyframe twice), or the slot count of prev_local_kf where that is
// larger.  first[] is part of the handle and is cleared by one memset at the head of every update, so no call sees an earlier one.
//
// sivo_localmap_apply keeps the handle current without sending the map again: a delta of replaced and appended rows goes up in one copy
// and the new tables are built from the old ones in the handle's second buffer (ping-pong, both grow-only), whose pointers take the
// place of the old ones under the handle's mutex once the call's one synchronisation has returned.  The per-item bodies and the check
// are localmap_delta_math.hpp.  For obs, slots, covisibles and children alike (blockIdx.y is the table):
// localmap_delta_mark_kernel    one thread per delta row: src[idx[j]] = j + 1 (src is zeroed, as long as the new row count).
// localmap_delta_len_kernel     one thread per new row: its length, summed per block of 256.
// localmap_delta_scan_kernel    the exclusive scan inside the block and the sum of the blocks before it, in one fixed order without
//                               atomics, into the new int64 offsets; the last row writes the table's total.
// localmap_delta_gather_kernel  one wave per new row copies it from the old pool or from the delta's, 64 entries at a time.
// localmap_delta_flags_kernel   point_bad, kf_bad, parent and kf_order are device-to-device copies of the old arrays; the delta's rows
//                               are scattered over them, and kf_order's tail is the appended indices where the caller gave no order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "localmap_handle.hpp"

namespace sivo {

constexpr int LV_THREADS = 1024;
constexpr int LS_THREADS = 1024;

__global__ __launch_bounds__(LV_THREADS) void localmap_vote_kernel(LmCall a) {
    __shared__ int32_t hist[SIVO_COVIS_LDS_KF];
    const int tid = threadIdx.x, n_kf = a.t.n_kf;
    const SivoObsTable o = lm_obs_table(a.t);
    if (n_kf <= SIVO_COVIS_LDS_KF) {
        for (int k = tid; k < n_kf; k += LV_THREADS) hist[k] = 0;
        __syncthreads();
        for (int i = tid; i < a.n_slots; i += LV_THREADS) {
            const int32_t p = a.frame_point[i];
            a.slot_cleared[i] = lm_slot_cleared(a.t, p);
            cv_count_slot(o, p, -1, [&](int32_t k) { atomicAdd(&hist[k], 1); });
        }
        __syncthreads();
        for (int k = tid; k < n_kf; k += LV_THREADS) a.counts[k] = hist[k];
    } else {
        for (int i = tid; i < a.n_slots; i += LV_THREADS) {
            const int32_t p = a.frame_point[i];
            a.slot_cleared[i] = lm_slot_cleared(a.t, p);
            cv_count_slot(o, p, -1, [&](int32_t k) { atomicAdd(&a.counts[k], 1); });
        }
    }
}

__global__ __launch_bounds__(LS_THREADS) void localmap_select_kernel(LmCall a) {
    __shared__ uint32_t marks_l[SIVO_COVIS_LDS_KF / 32];
    __shared__ int32_t wave_tot[LS_THREADS / 64];
    __shared__ unsigned long long best;
    __shared__ int32_t s_any, s_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_kf = a.t.n_kf;
    const bool lds_marks = n_kf <= SIVO_COVIS_LDS_KF;
    uint32_t *marks = lds_marks ? marks_l : a.marks_g;
    if (lds_marks)
        for (int w = tid; w < (n_kf + 31) / 32; w += LS_THREADS) marks_l[w] = 0;
    if (tid == 0) { best = 0; s_any = 0; s_n = 0; }
    __syncthreads();
    for (int i = tid; i < a.n_kf_pre; i += LS_THREADS) atomicOr(&marks[a.kf_pre[i] >> 5], lm_mark_bit(a.kf_pre[i]));
    for (int i = tid; i < a.n_pt_pre; i += LS_THREADS) a.first[a.pt_pre[i]] = LM_FIRST_PREMARKED;
    int any = 0;
    for (int k = tid; k < n_kf; k += LS_THREADS) any |= a.counts[k] > 0;
    if (any) s_any = 1;
    __syncthreads();
    const bool voted = s_any != 0;                                      // (:1144)

    // ---- stage 1 (:1156-1172): the voted keyframes that are not bad, in kf_order; n is the same in every thread
    int32_t n = 0;
    if (voted) {
        unsigned long long my_best = 0;
        for (int base = 0; base < n_kf; base += LS_THREADS) {
            const int i = base + tid;
            int32_t k = -1;
            bool take = false;
            if (i < n_kf) {
                k = a.t.kf_order[i];
                take = lm_stage1_takes(a.t, a.counts, k);
            }
            const unsigned long long b = __ballot(take);
            const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
            if (lane == 0) wave_tot[wave] = __popcll(b);
            __syncthreads();
            int32_t before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < LS_THREADS / 64; ++w) {
                const int32_t x = wave_tot[w];
                if (w < wave) before += x;
                total += x;
            }
            if (take) {
                a.local_kf[n + before + in_wave] = k;                   // (:1170)
                atomicOr(&marks[k >> 5], lm_mark_bit(k));               // (:1171)
                const unsigned long long key = lm_max_key(a.counts[k], i);
                if (key > my_best) my_best = key;                       // (:1165-1168)
            }
            n += total;
            __syncthreads();
        }
        if (my_best) atomicMax(&best, my_best);
    }
    __syncthreads();

    // ---- stage 2 (:1177-1229): wave 0, every lane on the same path
    if (wave == 0 && voted) {
        const int32_t n1 = n;                                           // itEndKF is taken before the loop
        int32_t m = n;
        auto push = [&](int32_t k) {
            if (lane == 0) a.local_kf[m] = k;
            marks[k >> 5] |= lm_mark_bit(k);                            // the same store in every lane: each lane reads its own later
            ++m;
        };
        for (int32_t j = 0; j < n1; ++j) {
            if (m > LM_MAX_LOCAL) break;                                // (:1183)
            const int32_t k = a.local_kf[j];
            {
                const int64_t c0 = a.t.covis_off[k];
                const int cn = (int)min((long long)(a.t.covis_off[k + 1] - c0), (long long)LM_BEST_COVIS);     // (:1189)
                int32_t c = -1;
                bool ok = false;
                if (lane < cn) {
                    c = a.t.covis_kf[c0 + lane];
                    ok = lm_neighbour_ok(a.t, marks, c);
                }
                const unsigned long long b = __ballot(ok);
                if (b) push(__shfl(c, __ffsll(b) - 1, 64));             // (:1197-1201)
            }
            for (int64_t cb = a.t.child_off[k], c1 = a.t.child_off[k + 1]; cb < c1; cb += 64) {
                int32_t c = -1;
                bool ok = false;
                if (cb + lane < c1) {
                    c = a.t.child_kf[cb + lane];
                    ok = lm_neighbour_ok(a.t, marks, c);
                }
                const unsigned long long b = __ballot(ok);
                if (b) {
                    push(__shfl(c, __ffsll(b) - 1, 64));                // (:1212-1216)
                    break;
                }
            }
            const int32_t par = a.t.parent[k];
            if (par >= 0 && !lm_marked(marks, par)) {                   // (:1222-1223: isBad() is not asked)
                push(par);
                break;                                                  // (:1226: leaves the loop over the keyframes)
            }
        }
        if (lane == 0) s_n = m;
    }
    __syncthreads();

    // ---- what the point passes walk: the new list, or the caller's where nobody voted (:1144-1145, then :1093)
    const int32_t n_list = voted ? s_n : a.n_prev;
    const int32_t *list = voted ? a.local_kf : a.prev;
    int32_t run = 0;
    for (int base = 0; base < n_list; base += LS_THREADS) {
        const int i = base + tid;
        int32_t cnt = 0;
        if (i < n_list) cnt = (int32_t)(a.t.slot_off[list[i] + 1] - a.t.slot_off[list[i]]);
        int32_t total;
        const int32_t excl = lm_block_excl_scan<LS_THREADS>(cnt, wave_tot, total);
        if (i < n_list) a.list_off[i] = run + excl;
        run += total;
    }
    if (tid == 0) {
        a.list_off[n_list] = run;
        a.hdr[LM_HDR_VOTED] = voted;
        a.hdr[LM_HDR_N_KF] = voted ? s_n : 0;
        a.hdr[LM_HDR_REF] = best ? a.t.kf_order[lm_key_pos(best)] : -1;  // (:1231)
        a.hdr[LM_HDR_N_LIST] = n_list;
        a.hdr[LM_HDR_G] = run;
    }
}

__global__ __launch_bounds__(LP_THREADS) void localmap_first_kernel(LmCall a) { lm_first_pass(a); }
__global__ __launch_bounds__(LP_THREADS) void localmap_count_kernel(LmCall a) { lm_count_pass(a); }
__global__ __launch_bounds__(LP_THREADS) void localmap_scatter_kernel(LmCall a) { lm_scatter_pass(a); }

struct LmBadArgs {
    uint8_t *point_bad, *kf_bad;
    int n_points, n_kf;
    const int32_t *point_idx, *kf_idx;
    const uint8_t *point_val, *kf_val;
};

__global__ __launch_bounds__(LP_THREADS) void localmap_set_bad_kernel(LmBadArgs a) {
    const int i = blockIdx.x * LP_THREADS + (int)threadIdx.x;
    if (i < a.n_points) a.point_bad[a.point_idx[i]] = a.point_val[i];
    else if (i - a.n_points < a.n_kf) a.kf_bad[a.kf_idx[i - a.n_points]] = a.kf_val[i - a.n_points];
}

// ---- sivo_localmap_apply: the new tables from the old ones and a delta of rows (localmap_delta_math.hpp) -----------------------------
struct LmdCall {
    LmdCsr c[LMD_TABLES];
    int32_t *block_sum[LMD_TABLES];        // one per block of LP_THREADS rows
    int64_t *totals;                       // LMD_TABLES: the new entry counts
    int32_t *src_p, *src_k;                // zeroed: n_points / n_kf (new)
    int32_t n_point_rows, n_kf_rows, n_kf_old, n_kf_new, order_given;
    const int32_t *point_idx, *kf_idx, *d_parent;
    const uint8_t *d_point_bad, *d_kf_bad;
    uint8_t *point_bad, *kf_bad;           // the new arrays: they hold a copy of the old ones when the flags kernel runs
    int32_t *parent, *kf_order;
};

__global__ __launch_bounds__(LP_THREADS) void localmap_delta_mark_kernel(LmdCall a) {
    const int i = blockIdx.x * LP_THREADS + (int)threadIdx.x;
    if (i < a.n_point_rows) lmd_mark(a.src_p, a.point_idx, i);
    else if (i - a.n_point_rows < a.n_kf_rows) lmd_mark(a.src_k, a.kf_idx, i - a.n_point_rows);
}

// pass 2a of the offsets: the rows of a block of LP_THREADS, summed.  blockIdx.y is the table.
__global__ __launch_bounds__(LP_THREADS) void localmap_delta_len_kernel(LmdCall a) {
    __shared__ int32_t wave_tot[LP_THREADS / 64];
    const LmdCsr &c = a.c[blockIdx.y];
    if ((int64_t)blockIdx.x * LP_THREADS >= c.n_new) return;            // the whole block
    const int64_t r = (int64_t)blockIdx.x * LP_THREADS + threadIdx.x;
    int32_t total;
    (void)lm_block_excl_scan<LP_THREADS>(r < c.n_new ? lmd_row_len(c, (int32_t)r) : 0, wave_tot, total);
    if (threadIdx.x == 0) a.block_sum[blockIdx.y][blockIdx.x] = total;
}

// x[0] + .. + x[n - 1], the same in every thread of the workgroup, summed in one fixed order: a strided partial sum per thread, a
// butterfly over the wave, the waves in order
__device__ inline int64_t lmd_block_base(const int32_t *x, int n, int64_t *wave_acc) {
    long long s = 0;
    for (int i = threadIdx.x; i < n; i += LP_THREADS) s += x[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0) wave_acc[threadIdx.x >> 6] = s;
    __syncthreads();
    int64_t r = 0;
#pragma unroll
    for (int w = 0; w < LP_THREADS / 64; ++w) r += wave_acc[w];
    __syncthreads();
    return r;
}

// pass 2b: the exclusive scan inside the block, the sum of the blocks before it; the last row writes the table's total
__global__ __launch_bounds__(LP_THREADS) void localmap_delta_scan_kernel(LmdCall a) {
    __shared__ int32_t wave_tot[LP_THREADS / 64];
    __shared__ int64_t wave_acc[LP_THREADS / 64];
    const int w = blockIdx.y, blk = blockIdx.x;
    const LmdCsr &c = a.c[w];
    if (c.n_new == 0) {
        if (blk == 0 && threadIdx.x == 0) a.totals[w] = 0;
        return;
    }
    if ((int64_t)blk * LP_THREADS >= c.n_new) return;                   // the whole block
    const int64_t r = (int64_t)blk * LP_THREADS + threadIdx.x;
    const int32_t len = r < c.n_new ? lmd_row_len(c, (int32_t)r) : 0;
    int32_t total;
    const int32_t excl = lm_block_excl_scan<LP_THREADS>(len, wave_tot, total);
    const int64_t base = lmd_block_base(a.block_sum[w], blk, wave_acc);
    if (r < c.n_new) c.new_off[r] = base + excl;
    if (r == c.n_new - 1) {
        c.new_off[c.n_new] = base + excl + len;
        a.totals[w] = base + excl + len;
    }
}

// one wave per new row: lane e takes the entries e, e + 64, ...
__global__ __launch_bounds__(LP_THREADS) void localmap_delta_gather_kernel(LmdCall a) {
    const LmdCsr &c = a.c[blockIdx.y];
    const int64_t r = (int64_t)blockIdx.x * (LP_THREADS / 64) + (threadIdx.x >> 6);
    if (r >= c.n_new) return;
    const int lane = threadIdx.x & 63;
    const int64_t at = c.new_off[r];
    const int32_t len = (int32_t)(c.new_off[r + 1] - at);
    const int32_t *from = lmd_row_source(c, (int32_t)r);
    for (int32_t e = lane; e < len; e += 64) c.new_val[at + e] = from[e];
}

// the delta's flags and parents over the copies of the old arrays; kf_order's tail where the caller gave no order
__global__ __launch_bounds__(LP_THREADS) void localmap_delta_flags_kernel(LmdCall a) {
    int i = blockIdx.x * LP_THREADS + (int)threadIdx.x;
    if (i < a.n_point_rows) { a.point_bad[a.point_idx[i]] = a.d_point_bad[i] ? 1 : 0; return; }
    i -= a.n_point_rows;
    if (i < a.n_kf_rows) {
        a.kf_bad[a.kf_idx[i]] = a.d_kf_bad[i] ? 1 : 0;
        a.parent[a.kf_idx[i]] = a.d_parent[i];
        return;
    }
    i -= a.n_kf_rows;
    if (!a.order_given && i < a.n_kf_new - a.n_kf_old) a.kf_order[a.n_kf_old + i] = a.n_kf_old + i;
}

}  // namespace sivo

using namespace sivo;

// the checked tables into the handle's buffer: one copy, synchronised before it returns
static void lm_load(sivo_localmap *m, const SivoLocalMapTables &t) {
    const size_t K = (size_t)t.n_kf, P = (size_t)t.n_points;
    const size_t no = P ? (size_t)t.obs_off[P] : 0, ns = K ? (size_t)t.slot_off[K] : 0, nc = K ? (size_t)t.covis_off[K] : 0,
                 nh = K ? (size_t)t.child_off[K] : 0;
    std::vector<int32_t> identity;
    if (!t.kf_order) {
        identity.resize(K);
        for (size_t k = 0; k < K; ++k) identity[k] = (int32_t)k;
    }
    SolverCtx &c = lm_ctx();
    SivoLocalMapTables d{};
    uint32_t *first = nullptr;
    Layout L;
    d.n_kf = t.n_kf; d.n_points = t.n_points;
    L.copy(d.obs_off, t.obs_off, P ? 8 * (P + 1) : 0); L.copy(d.obs_kf, t.obs_kf, 4 * no); L.copy(d.point_bad, t.point_bad, P);
    L.copy(d.kf_bad, t.kf_bad, K); L.copy(d.slot_off, t.slot_off, K ? 8 * (K + 1) : 0); L.copy(d.slot_point, t.slot_point, 4 * ns);
    L.copy(d.covis_off, t.covis_off, K ? 8 * (K + 1) : 0); L.copy(d.covis_kf, t.covis_kf, 4 * nc);
    L.copy(d.child_off, t.child_off, K ? 8 * (K + 1) : 0); L.copy(d.child_kf, t.child_kf, 4 * nh); L.copy(d.parent, t.parent, 4 * K);
    L.copy(d.kf_order, t.kf_order ? t.kf_order : identity.data(), 4 * K);
    L.take(first, 4 * P);
    std::vector<char> host(L.staged());
    L.place(m->dev(m->cur).reserve(L.bytes()), host.data());
    L.send(c.stream);
    SIVO_HIP(hipStreamSynchronize(c.stream));
    m->attr_reserve(P, 0, c.stream);                                    // (no row survives: the caller may have renumbered)
    m->attr_unset_all(P);
    m->d = d;
    m->first = first;
    m->slot_off.assign(K + 1, 0);
    if (K) std::memcpy(m->slot_off.data(), t.slot_off, 8 * (K + 1));
    m->total_slots = (int64_t)ns;
    m->total[LMD_OBS] = (int64_t)no; m->total[LMD_SLOT] = (int64_t)ns; m->total[LMD_COVIS] = (int64_t)nc; m->total[LMD_CHILD] = (int64_t)nh;
}

extern "C" int sivo_localmap_create(const SivoLocalMapTables *t, sivo_localmap_t *map) {
    return guarded([&] {
        if (!map) throw std::invalid_argument("sivo_localmap_create: null handle pointer");
        *map = nullptr;
        lm_throw("sivo_localmap_create", lm_check_tables(t));
        require_device();
        sivo_localmap *m = new sivo_localmap;
        try {
            SIVO_HIP(hipGetDevice(&m->device));
            lm_load(m, *t);
        } catch (...) {
            delete m;
            throw;
        }
        *map = m;
        return SIVO_OK;
    });
}

extern "C" int sivo_localmap_replace(sivo_localmap_t m, const SivoLocalMapTables *t) {
    return guarded([&] {
        if (!m) throw std::invalid_argument("sivo_localmap_replace: null handle");
        lm_throw("sivo_localmap_replace", lm_check_tables(t));
        std::lock_guard<std::mutex> lock(m->mu);
        DeviceGuard dg(m->device);
        lm_load(m, *t);
        return SIVO_OK;
    });
}

extern "C" int sivo_localmap_destroy(sivo_localmap_t m) {
    return guarded([&] {
        if (!m) return SIVO_OK;
        {
            DeviceGuard dg(m->device);
            m->dev(0).release();
            m->dev(1).release();
            m->attr_release();
        }
        delete m;
        return SIVO_OK;
    });
}

extern "C" int sivo_localmap_set_bad(sivo_localmap_t m, int n_points, const int32_t *point_idx, const uint8_t *point_val, int n_kf,
                                     const int32_t *kf_idx, const uint8_t *kf_val) {
    return guarded([&] {
        if (!m) throw std::invalid_argument("sivo_localmap_set_bad: null handle");
        std::lock_guard<std::mutex> lock(m->mu);
        lm_throw("sivo_localmap_set_bad", lm_check_set_bad(m->d.n_kf, m->d.n_points, n_points, point_idx, point_val, n_kf, kf_idx, kf_val));
        if (n_points == 0 && n_kf == 0) return SIVO_OK;
        // of an index listed twice the later entry holds: the scatter sees every index once
        std::map<int32_t, uint8_t> pm, km;
        for (int i = 0; i < n_points; ++i) pm[point_idx[i]] = point_val[i] ? 1 : 0;
        for (int i = 0; i < n_kf; ++i) km[kf_idx[i]] = kf_val[i] ? 1 : 0;
        std::vector<int32_t> pi, ki;
        std::vector<uint8_t> pv, kv;
        for (const auto &e : pm) { pi.push_back(e.first); pv.push_back(e.second); }
        for (const auto &e : km) { ki.push_back(e.first); kv.push_back(e.second); }
        DeviceGuard dg(m->device);
        SolverCtx &c = lm_ctx();
        LmBadArgs a;
        Layout L;
        L.copy(a.point_idx, pi.data(), 4 * pi.size()); L.copy(a.point_val, pv.data(), pv.size());
        L.copy(a.kf_idx, ki.data(), 4 * ki.size()); L.copy(a.kf_val, kv.data(), kv.size());
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        a.point_bad = const_cast<uint8_t *>(m->d.point_bad); a.kf_bad = const_cast<uint8_t *>(m->d.kf_bad);
        a.n_points = (int)pi.size(); a.n_kf = (int)ki.size();
        L.send(c.stream);
        hipLaunchKernelGGL(localmap_set_bad_kernel, dim3((unsigned)cdiv(a.n_points + a.n_kf, LP_THREADS)), dim3(LP_THREADS), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipStreamSynchronize(c.stream));
        return SIVO_OK;
    });
}

// The device part of sivo_localmap_update (localmap_handle.hpp): the caller holds the handle's mutex and has checked the arguments.
int sivo::lm_run_update(sivo_localmap *m, const LmUpdateArgs &u, int64_t g_prev, const char *who, LmUpdateHook *hook, LmCall *call) {
    require_device();
    DeviceGuard dg(m->device);
    SolverCtx &c = lm_ctx();
    const size_t K = (size_t)m->d.n_kf, P = (size_t)m->d.n_points, S = (size_t)u.n_slots;
    const int64_t g_max = std::max(m->total_slots, g_prev);             // no list the point passes walk holds more slots
    const unsigned nb = (unsigned)std::max<int64_t>(1, cdiv64(g_max, LP_THREADS));
    LmCall a;
    a.t = m->d; a.first = m->first;
    a.n_slots = u.n_slots; a.n_kf_pre = u.n_kf_premarked; a.n_pt_pre = u.n_point_premarked; a.n_prev = u.n_prev;
    a.point_cap = (int)std::min<int64_t>(u.point_capacity, std::min<int64_t>((int64_t)P, g_max));
    Layout L;
    L.copy(a.frame_point, u.frame_point, 4 * S); L.copy(a.kf_pre, u.kf_premarked, 4 * (size_t)u.n_kf_premarked);
    L.copy(a.pt_pre, u.point_premarked, 4 * (size_t)u.n_point_premarked); L.copy(a.prev, u.prev_local_kf, 4 * (size_t)u.n_prev);
    L.zero(a.marks_g, K > SIVO_COVIS_LDS_KF ? 4 * ((K + 31) / 32) : 0); L.zero(a.counts, 4 * K);
    L.take(a.hdr, 4 * LM_HDR_WORDS); L.take(a.slot_cleared, S); L.take(a.local_kf, 4 * K); L.take(a.local_point, 4 * (size_t)a.point_cap);
    L.take(a.list_off, 4 * (std::max(K, (size_t)u.n_prev) + 1)); L.take(a.block_sum, 4 * (size_t)nb);       // scratch: not copied back
    if (hook) hook->regions(L);
    L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
    L.send(c.stream);
    if (P) SIVO_HIP(hipMemsetAsync(m->first, 0xFF, 4 * P, c.stream));
    hipLaunchKernelGGL(localmap_vote_kernel, dim3(1), dim3(LV_THREADS), 0, c.stream, a);
    hipLaunchKernelGGL(localmap_select_kernel, dim3(1), dim3(LS_THREADS), 0, c.stream, a);
    hipLaunchKernelGGL(localmap_first_kernel, dim3(nb), dim3(LP_THREADS), 0, c.stream, a);
    hipLaunchKernelGGL(localmap_count_kernel, dim3(nb), dim3(LP_THREADS), 0, c.stream, a);
    hipLaunchKernelGGL(localmap_scatter_kernel, dim3(nb), dim3(LP_THREADS), 0, c.stream, a);
    SIVO_HIP(hipGetLastError());
    if (hook) hook->launch(a, c.stream);
    const size_t down = (size_t)((const char *)a.local_point - (const char *)a.counts) + 4 * (size_t)a.point_cap;
    SIVO_HIP(hipMemcpyAsync(L.host(a.counts), a.counts, down, hipMemcpyDeviceToHost, c.stream));
    SIVO_HIP(hipStreamSynchronize(c.stream));
    const int32_t *hdr = L.host(a.hdr);
    const int32_t v = hdr[LM_HDR_VOTED], nk = hdr[LM_HDR_N_KF], np = hdr[LM_HDR_N_POINTS];
    if (v && nk > u.kf_capacity) return fail(SIVO_ERR_CAPACITY, "%s: %d local keyframes, capacity %d", who, nk, u.kf_capacity);
    if (np > u.point_capacity) return fail(SIVO_ERR_CAPACITY, "%s: %d local map points, capacity %d", who, np, u.point_capacity);
    *u.voted = v;
    if (S) std::memcpy(u.slot_cleared, L.host(a.slot_cleared), S);
    if (v) {
        *u.n_local_kf = nk;
        if (nk) std::memcpy(u.local_kf, L.host(a.local_kf), 4 * (size_t)nk);
    }
    *u.ref_kf = hdr[LM_HDR_REF];
    *u.n_local_points = np;
    if (np) std::memcpy(u.local_point, L.host(a.local_point), 4 * (size_t)np);
    if (u.counts && K) std::memcpy(u.counts, L.host(a.counts), 4 * K);
    if (call) *call = a;
    return SIVO_OK;
}

extern "C" int sivo_localmap_update(sivo_localmap_t m, int n_slots, const int32_t *frame_point, int n_kf_premarked,
                                    const int32_t *kf_premarked, int n_point_premarked, const int32_t *point_premarked, int n_prev,
                                    const int32_t *prev_local_kf, int32_t *voted, uint8_t *slot_cleared, int kf_capacity,
                                    int32_t *local_kf, int32_t *n_local_kf, int32_t *ref_kf, int point_capacity, int32_t *local_point,
                                    int32_t *n_local_points, int32_t *counts) {
    return guarded([&] {
        if (!m) throw std::invalid_argument("sivo_localmap_update: null handle");
        std::lock_guard<std::mutex> lock(m->mu);
        int64_t g_prev = 0;
        lm_throw("sivo_localmap_update",
                 lm_check_update(m->d.n_kf, m->d.n_points, m->slot_off.data(), n_slots, frame_point, n_kf_premarked, kf_premarked, n_point_premarked,
                                 point_premarked, n_prev, prev_local_kf, voted, slot_cleared, kf_capacity, local_kf, n_local_kf, ref_kf,
                                 point_capacity, local_point, n_local_points, &g_prev));
        const LmUpdateArgs u{n_slots, frame_point, n_kf_premarked, kf_premarked, n_point_premarked, point_premarked, n_prev, prev_local_kf, voted,
                             slot_cleared, kf_capacity, local_kf, n_local_kf, ref_kf, point_capacity, local_point, n_local_points, counts};
        return lm_run_update(m, u, g_prev, "sivo_localmap_update", nullptr, nullptr);
    });
}

// The delta's rows in one upload, the four passes over each table, the flags and the order, the four totals back: one synchronisation.
// The new tables are built in the handle's other buffer; the handle changes only after everything has succeeded.
extern "C" int sivo_localmap_apply(sivo_localmap_t m, const SivoLocalMapDelta *dl) {
    return guarded([&] {
        if (!m) throw std::invalid_argument("sivo_localmap_apply: null handle");
        std::lock_guard<std::mutex> lock(m->mu);
        lm_throw("sivo_localmap_apply", lmd_check_delta(m->d.n_kf, m->d.n_points, m->total, dl, sizeof(SivoLocalMapDelta)));
        if (lmd_is_empty(m->d.n_kf, m->d.n_points, *dl)) return SIVO_OK;
        require_device();
        DeviceGuard dg(m->device);
        SolverCtx &c = lm_ctx();
        const SivoLocalMapDelta &d = *dl;
        const size_t K0 = (size_t)m->d.n_kf, P0 = (size_t)m->d.n_points, K1 = (size_t)d.n_kf, P1 = (size_t)d.n_points;
        const size_t np = (size_t)d.n_point_rows, nk = (size_t)d.n_kf_rows;
        const int32_t rows_old[LMD_TABLES] = {(int32_t)P0, (int32_t)K0, (int32_t)K0, (int32_t)K0};
        const int32_t rows_new[LMD_TABLES] = {(int32_t)P1, (int32_t)K1, (int32_t)K1, (int32_t)K1};
        const int64_t *old_off[LMD_TABLES] = {m->d.obs_off, m->d.slot_off, m->d.covis_off, m->d.child_off};
        const int32_t *old_val[LMD_TABLES] = {m->d.obs_kf, m->d.slot_point, m->d.covis_kf, m->d.child_kf};
        LmdCall a{};
        const int32_t *d_order = nullptr;
        unsigned nb[LMD_TABLES], nb_max = 1;
        Layout L;                                                       // the call's staging: the delta, the marks, the block sums, the totals
        L.copy(a.point_idx, d.point_idx, 4 * np); L.copy(a.d_point_bad, d.point_bad, np);
        L.copy(a.kf_idx, d.kf_idx, 4 * nk); L.copy(a.d_kf_bad, d.kf_bad, nk); L.copy(a.d_parent, d.kf_parent, 4 * nk);
        size_t bound[LMD_TABLES];                                       // old total + delta total: what the new pools are allocated from
        for (int w = 0; w < LMD_TABLES; ++w) {
            const int64_t *off;
            const int32_t *val;
            lmd_delta_table(d, w, off, val);
            const size_t rows = w == LMD_OBS ? np : nk, entries = rows ? (size_t)off[rows] : 0;
            L.copy(a.c[w].d_off, off, rows ? 8 * (rows + 1) : 0); L.copy(a.c[w].d_val, val, 4 * entries);
            bound[w] = (size_t)m->total[w] + entries;
            nb[w] = (unsigned)std::max(1, cdiv(rows_new[w], LP_THREADS));
            nb_max = std::max(nb_max, nb[w]);
        }
        L.copy(d_order, d.kf_order, d.kf_order ? 4 * K1 : 0);
        L.zero(a.src_p, 4 * P1); L.zero(a.src_k, 4 * K1);
        for (int w = 0; w < LMD_TABLES; ++w) L.take(a.block_sum[w], 4 * (size_t)nb[w]);
        L.take(a.totals, 8 * LMD_TABLES);
        SivoLocalMapTables n{};                                         // the new tables, in the buffer the handle does not use
        uint32_t *first = nullptr;
        Layout N;
        n.n_kf = d.n_kf; n.n_points = d.n_points;
        N.take(n.obs_off, P1 ? 8 * (P1 + 1) : 0); N.take(n.obs_kf, 4 * bound[LMD_OBS]); N.take(n.point_bad, P1);
        N.take(n.kf_bad, K1); N.take(n.slot_off, K1 ? 8 * (K1 + 1) : 0); N.take(n.slot_point, 4 * bound[LMD_SLOT]);
        N.take(n.covis_off, K1 ? 8 * (K1 + 1) : 0); N.take(n.covis_kf, 4 * bound[LMD_COVIS]);
        N.take(n.child_off, K1 ? 8 * (K1 + 1) : 0); N.take(n.child_kf, 4 * bound[LMD_CHILD]); N.take(n.parent, 4 * K1);
        N.take(n.kf_order, 4 * K1); N.take(first, 4 * P1);
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        N.place(m->dev(1 - m->cur).reserve(N.bytes()), nullptr);
        m->attr_reserve(P1, P0, c.stream);                              // the stored rows move with a device copy; capacity only
        int64_t *new_off[LMD_TABLES] = {const_cast<int64_t *>(n.obs_off), const_cast<int64_t *>(n.slot_off), const_cast<int64_t *>(n.covis_off),
                                        const_cast<int64_t *>(n.child_off)};
        int32_t *new_val[LMD_TABLES] = {const_cast<int32_t *>(n.obs_kf), const_cast<int32_t *>(n.slot_point), const_cast<int32_t *>(n.covis_kf),
                                        const_cast<int32_t *>(n.child_kf)};
        for (int w = 0; w < LMD_TABLES; ++w) {
            a.c[w].n_old = rows_old[w]; a.c[w].n_new = rows_new[w]; a.c[w].old_off = old_off[w]; a.c[w].old_val = old_val[w];
            a.c[w].src = w == LMD_OBS ? a.src_p : a.src_k; a.c[w].new_off = new_off[w]; a.c[w].new_val = new_val[w];
        }
        a.n_point_rows = (int32_t)np; a.n_kf_rows = (int32_t)nk; a.n_kf_old = (int32_t)K0; a.n_kf_new = (int32_t)K1; a.order_given = d.kf_order ? 1 : 0;
        a.point_bad = const_cast<uint8_t *>(n.point_bad); a.kf_bad = const_cast<uint8_t *>(n.kf_bad);
        a.parent = const_cast<int32_t *>(n.parent); a.kf_order = const_cast<int32_t *>(n.kf_order);
        L.send(c.stream);
        if (P0) SIVO_HIP(hipMemcpyAsync(a.point_bad, m->d.point_bad, P0, hipMemcpyDeviceToDevice, c.stream));
        if (K0) {
            SIVO_HIP(hipMemcpyAsync(a.kf_bad, m->d.kf_bad, K0, hipMemcpyDeviceToDevice, c.stream));
            SIVO_HIP(hipMemcpyAsync(a.parent, m->d.parent, 4 * K0, hipMemcpyDeviceToDevice, c.stream));
        }
        if (d.kf_order) SIVO_HIP(hipMemcpyAsync(a.kf_order, d_order, 4 * K1, hipMemcpyDeviceToDevice, c.stream));
        else if (K0) SIVO_HIP(hipMemcpyAsync(a.kf_order, m->d.kf_order, 4 * K0, hipMemcpyDeviceToDevice, c.stream));
        const unsigned rows_max = (unsigned)std::max<size_t>(1, std::max(P1, K1));
        if (np + nk) hipLaunchKernelGGL(localmap_delta_mark_kernel, dim3((unsigned)cdiv64((int64_t)(np + nk), LP_THREADS)), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(localmap_delta_len_kernel, dim3(nb_max, LMD_TABLES), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(localmap_delta_scan_kernel, dim3(nb_max, LMD_TABLES), dim3(LP_THREADS), 0, c.stream, a);
        hipLaunchKernelGGL(localmap_delta_gather_kernel, dim3((unsigned)cdiv64(rows_max, LP_THREADS / 64), LMD_TABLES), dim3(LP_THREADS), 0, c.stream, a);
        const size_t n_flags = np + nk + (d.kf_order ? 0 : K1 - K0);
        if (n_flags) hipLaunchKernelGGL(localmap_delta_flags_kernel, dim3((unsigned)cdiv64((int64_t)n_flags, LP_THREADS)), dim3(LP_THREADS), 0, c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipMemcpyAsync(L.host(a.totals), a.totals, 8 * LMD_TABLES, hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        const int64_t *totals = L.host(a.totals);
        std::vector<int64_t> slot_off = lmd_host_slot_off(m->slot_off, (int32_t)K0, d);      // O(keyframes), on the host
        if (totals[LMD_SLOT] != slot_off.back()) throw std::logic_error("sivo_localmap_apply: the device's slot total differs from the host's");
        for (int w = 0; w < LMD_TABLES; ++w) m->total[w] = totals[w];   // the exact totals, not the bounds the pools were sized from
        m->d = n;
        m->first = first;
        m->attr_resize(P1);                                             // appended points are unset
        m->slot_off.swap(slot_off);
        m->total_slots = m->total[LMD_SLOT];
        m->cur = 1 - m->cur;
        return SIVO_OK;
    });
}

extern "C" int sivo_localmap_sizes(sivo_localmap_t m, int64_t out[6]) {
    return guarded([&] {
        if (!m) throw std::invalid_argument("sivo_localmap_sizes: null handle");
        if (!out) throw std::invalid_argument("sivo_localmap_sizes: null out");
        std::lock_guard<std::mutex> lock(m->mu);
        out[0] = m->d.n_kf; out[1] = m->d.n_points;
        for (int w = 0; w < LMD_TABLES; ++w) out[2 + w] = m->total[w];
        return SIVO_OK;
    });
}

extern "C" int sivo_localmap_export(sivo_localmap_t m, SivoLocalMapTables *out) {
    return guarded([&] {
        if (!m) throw std::invalid_argument("sivo_localmap_export: null handle");
        std::lock_guard<std::mutex> lock(m->mu);
        lm_throw("sivo_localmap_export", lmd_check_export(m->d.n_kf, m->d.n_points, m->total, out));
        const size_t K = (size_t)m->d.n_kf, P = (size_t)m->d.n_points;
        if (K == 0 && P == 0) return SIVO_OK;
        require_device();
        DeviceGuard dg(m->device);
        SolverCtx &c = lm_ctx();
        auto down = [&](const void *dst, const void *src, size_t bytes) {
            if (bytes) SIVO_HIP(hipMemcpyAsync(const_cast<void *>(dst), src, bytes, hipMemcpyDeviceToHost, c.stream));
        };
        down(out->obs_off, m->d.obs_off, P ? 8 * (P + 1) : 0); down(out->obs_kf, m->d.obs_kf, 4 * (size_t)m->total[LMD_OBS]);
        down(out->point_bad, m->d.point_bad, P); down(out->kf_bad, m->d.kf_bad, K);
        down(out->slot_off, m->d.slot_off, K ? 8 * (K + 1) : 0); down(out->slot_point, m->d.slot_point, 4 * (size_t)m->total[LMD_SLOT]);
        down(out->covis_off, m->d.covis_off, K ? 8 * (K + 1) : 0); down(out->covis_kf, m->d.covis_kf, 4 * (size_t)m->total[LMD_COVIS]);
        down(out->child_off, m->d.child_off, K ? 8 * (K + 1) : 0); down(out->child_kf, m->d.child_kf, 4 * (size_t)m->total[LMD_CHILD]);
        down(out->parent, m->d.parent, 4 * K); down(out->kf_order, m->d.kf_order, 4 * K);
        SIVO_HIP(hipStreamSynchronize(c.stream));
        return SIVO_OK;
    });
}
