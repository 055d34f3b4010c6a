// bow.hip — DBoW2's bag-of-words transform and the keyframe database's inverted-file walk on the device (reference
// dependencies/DBoW2/DBoW2/TemplatedVocabulary.h:1126-1259, src/orbslam/KeyFrameDatabase.cc:72-322).  Three kernels:
//   * bow_descend_kernel: the descent, L dependent gathers per feature, each behind a cache or HBM miss — latency bound, so spread over
//     the chip: BOW_GROUP lanes per feature, each lane loading one child's 32 bytes as two 16-byte loads (a loop when k > BOW_GROUP),
//     reduced to (min distance, lowest child index) by shuffles; every set of a batch in one launch;
//   * bow_set_kernel: one workgroup per set with the keys in LDS: bitonic sort of (word, feature), run lengths, the value of a word by
//     repeated addition, the L1 norm summed by ONE lane in ascending word order (bit-identity with BowVector::normalize), the division;
//     then the same sort by (node, feature) for the FeatureVector's CSR form;
//   * bow_query_kernel: one wavefront per stored vector, the query's sorted words in LDS: every lane looks one stored word up by binary
//     search, the terms of the shared words are added in ascending word order (a ballot, then the set lanes in turn).
// Arithmetic: bow_math.hpp, which g++ also compiles for the host; tests/bow_restatement.py restates it and is compared bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "bow_voc.hpp"
#include "common.hpp"
#include "solver_host.hpp"

#pragma clang fp contract(off)

namespace sivo {

constexpr int BOW_GROUP = 16;          // lanes per feature in the descent (ORBvoc.txt: k = 10)
constexpr int BOW_THREADS = 256;
constexpr int BOW_QUERY_WAVES = BOW_THREADS / 64;
static_assert(SIVO_BOW_SET_CAP == BOW_SET_CAP, "the header's cap is the kernels' cap");

struct BowSetDesc { int64_t off; int32_t n, pad_; };

struct BowArgs {
    BowVocView v;
    const uint32_t *desc;      // 8 words per feature
    const BowSetDesc *sets;
    int32_t total, levelsup, npad_max;
    int32_t *word, *node, *leaf;                     // per feature
    int32_t *bow_words, *n_words;
    double *bow_values;
    int32_t *fv_nodes, *fv_off, *fv_feat, *n_fv;
#ifdef SIVO_DIAG
    int64_t *stamps;                                 // diagnostic build: per set, wall-clock ticks of the set's workgroup and of its norm loop
#endif
};

__global__ __launch_bounds__(BOW_THREADS) void bow_descend_kernel(BowArgs a) {
    const int f = (int)((blockIdx.x * (unsigned)BOW_THREADS + threadIdx.x) / BOW_GROUP);
    const int lane = (int)threadIdx.x & (BOW_GROUP - 1);
    if (f >= a.total) return;                                       // (a whole group leaves together)
    const uint4 *fp = reinterpret_cast<const uint4 *>(a.desc) + 2 * (int64_t)f;
    const uint4 f0 = fp[0], f1 = fp[1];
    const uint32_t fd[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
    const int nid_level = a.v.L - a.levelsup;
    int32_t node = 0, at = nid_level <= 0 ? 0 : -1;
    int level = 0;
    for (;;) {
        const BowKids k = a.v.kids[node];
        if (k.count == 0) break;
        ++level;
        uint32_t best = 0xFFFFFFFFu;
        for (int c = lane; c < k.count; c += BOW_GROUP) {
            const uint4 *cp = reinterpret_cast<const uint4 *>(a.v.cdesc) + 2 * (int64_t)(k.first + c);
            const uint4 c0 = cp[0], c1 = cp[1];
            const uint32_t cd[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
            const uint32_t key = bow_child_key(bow_distance(fd, cd), c);
            best = key < best ? key : best;
        }
        for (int m = BOW_GROUP / 2; m > 0; m >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)best, m, BOW_GROUP);
            best = o < best ? o : best;
        }
        node = a.v.cnode[k.first + (int)(best & 0xFFu)];
        if (level == nid_level) at = node;
    }
    if (lane == 0) {
        a.leaf[f] = node;
        a.word[f] = a.v.word[node];
        a.node[f] = at < 0 ? node : at;
    }
}

// K[0 .. npad) ascending, npad a power of two
__device__ void bow_sort(uint64_t *K, int npad) {
    const int tid = (int)threadIdx.x;
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npad; i += BOW_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const uint64_t p = K[i], q = K[x];
                    if ((p > q) == ((i & k) == 0)) { K[i] = q; K[x] = p; }
                }
            }
            __syncthreads();
        }
}

// Exclusive prefix of `mine` over the workgroup; *total = the sum.  scan: BOW_THREADS ints of LDS.
__device__ int bow_scan(int *scan, int mine, int *total) {
    const int tid = (int)threadIdx.x;
    __syncthreads();
    scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < BOW_THREADS; d <<= 1) {
        const int t = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += t;
        __syncthreads();
    }
    *total = scan[BOW_THREADS - 1];
    return scan[tid] - mine;
}

__global__ __launch_bounds__(BOW_THREADS) void bow_set_kernel(BowArgs a) {
    extern __shared__ uint64_t bow_lds[];
    __shared__ int scan[BOW_THREADS];
    __shared__ int s_m;
    __shared__ double s_norm;
    uint64_t *K = bow_lds;
    double *V = reinterpret_cast<double *>(bow_lds + a.npad_max);
    const int tid = (int)threadIdx.x, s = (int)blockIdx.x;
#ifdef SIVO_DIAG
    const int64_t t_begin = (int64_t)wall_clock64();
    int64_t t_norm = 0;
#endif
    const BowSetDesc sd = a.sets[s];
    const int n = sd.n;
    const int64_t off = sd.off;
    int32_t *fv_off = a.fv_off + off + s;
    if (n == 0) {
        if (tid == 0) {
            a.n_words[s] = 0; a.n_fv[s] = 0; fv_off[0] = 0;
#ifdef SIVO_DIAG
            a.stamps[2 * s] = 0; a.stamps[2 * s + 1] = 0;
#endif
        }
        return;
    }
    int npad = 1;
    while (npad < n) npad <<= 1;
    const int chunk = npad > BOW_THREADS ? npad / BOW_THREADS : 1;
    if (tid == 0) s_m = 0;
    __syncthreads();
    // ---- the BowVector: keys (word, feature), the stopped features last
    for (int i = tid; i < npad; i += BOW_THREADS) {
        uint64_t key = ~0ull;
        if (i < n && !bow_stopped(a.v.weight[a.leaf[off + i]])) {
            key = ((uint64_t)(uint32_t)a.word[off + i] << 32) | (uint32_t)i;
            atomicAdd(&s_m, 1);
        }
        K[i] = key;
    }
    __syncthreads();
    const int m = s_m;
    bow_sort(K, npad);
    const int lo = min(tid * chunk, m), hi = min(lo + chunk, m);
    int heads = 0;
    for (int i = lo; i < hi; ++i) heads += i == 0 || (K[i] >> 32) != (K[i - 1] >> 32);
    int nu;
    int u = bow_scan(scan, heads, &nu);
    for (int i = lo; i < hi; ++i) {
        const uint32_t w = (uint32_t)(K[i] >> 32);
        if (i > 0 && (uint32_t)(K[i - 1] >> 32) == w) continue;
        int j = i + 1;
        while (j < m && (uint32_t)(K[j] >> 32) == w) ++j;
        V[u] = bow_repeat_add(a.v.weight[a.leaf[off + (uint32_t)K[i]]], j - i);       // addWeight, once per occurrence
        a.bow_words[off + u] = (int32_t)w;
        ++u;
    }
    __syncthreads();
    if (tid == 0) {                                                  // BowVector::normalize: one lane, ascending word order
#ifdef SIVO_DIAG
        const int64_t t0 = (int64_t)wall_clock64();
#endif
        s_norm = bow_l1_norm(V, nu);
#ifdef SIVO_DIAG
        t_norm = (int64_t)wall_clock64() - t0;
#endif
    }
    __syncthreads();
    const double norm = s_norm;
    for (int i = tid; i < nu; i += BOW_THREADS) a.bow_values[off + i] = norm > 0.0 ? V[i] / norm : V[i];
    if (tid == 0) a.n_words[s] = nu;
    __syncthreads();
    // ---- the FeatureVector: keys (node, feature)
    for (int i = tid; i < npad; i += BOW_THREADS) {
        uint64_t key = ~0ull;
        if (i < n && !bow_stopped(a.v.weight[a.leaf[off + i]])) key = ((uint64_t)(uint32_t)a.node[off + i] << 32) | (uint32_t)i;
        K[i] = key;
    }
    __syncthreads();
    bow_sort(K, npad);
    heads = 0;
    for (int i = lo; i < hi; ++i) heads += i == 0 || (K[i] >> 32) != (K[i - 1] >> 32);
    u = bow_scan(scan, heads, &nu);
    for (int i = lo; i < hi; ++i) {
        a.fv_feat[off + i] = (int32_t)(uint32_t)K[i];
        if (i > 0 && (K[i - 1] >> 32) == (K[i] >> 32)) continue;
        a.fv_nodes[off + u] = (int32_t)(K[i] >> 32);
        fv_off[u] = i;
        ++u;
    }
    if (tid == 0) {
        fv_off[nu] = m;
        a.n_fv[s] = nu;
#ifdef SIVO_DIAG
        a.stamps[2 * s] = (int64_t)wall_clock64() - t_begin;
        a.stamps[2 * s + 1] = t_norm;
#endif
    }
}

// The vocabulary's image on the current device: uploaded by the first call that needs it.
static const BowVocView &bow_voc_on_device(sivo_voc *voc) {
    std::lock_guard<std::mutex> lock(voc->mutex);
    int d = 0;
    SIVO_HIP(hipGetDevice(&d));
    if (voc->d_base) {
        if (voc->device != d) throw std::invalid_argument("vocabulary: its image lives on another device than the current one");
        return voc->dev;
    }
    const BowVocImage &img = voc->img;
    auto up = [](size_t bytes) { return (std::max<size_t>(bytes, 8) + 255) / 256 * 256; };
    const size_t b0 = up(img.kids.size() * sizeof(BowKids)), b1 = up(img.cdesc.size() * 4), b2 = up(img.cnode.size() * 4),
                 b3 = up(img.word.size() * 4), b4 = up(img.weight.size() * 8);
    char *base = nullptr;
    SIVO_HIP(hipMalloc((void **)&base, b0 + b1 + b2 + b3 + b4));
    const struct { size_t off; const void *src; size_t bytes; } parts[5] = {
        {0, img.kids.data(), img.kids.size() * sizeof(BowKids)}, {b0, img.cdesc.data(), img.cdesc.size() * 4},
        {b0 + b1, img.cnode.data(), img.cnode.size() * 4}, {b0 + b1 + b2, img.word.data(), img.word.size() * 4},
        {b0 + b1 + b2 + b3, img.weight.data(), img.weight.size() * 8}};
    for (const auto &part : parts) {
        if (!part.bytes) continue;
        const hipError_t e = hipMemcpy(base + part.off, part.src, part.bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {                                         // nothing is published: the next call starts over
            (void)hipFree(base);
            SIVO_HIP(e);
        }
    }
    voc->dev = BowVocView{(const BowKids *)base, (const uint32_t *)(base + b0), (const int32_t *)(base + b0 + b1),
                          (const int32_t *)(base + b0 + b1 + b2), (const double *)(base + b0 + b1 + b2 + b3), img.L};
    voc->device = d;
    voc->d_base = base;                                                // published last, after every copy succeeded
    return voc->dev;
}

#ifdef SIVO_DIAG
static thread_local double bow_last_set_us = 0.0, bow_last_norm_us = 0.0;
#endif

static int bow_run(sivo_voc *voc, const uint8_t *desc, const int64_t *offsets, int n_sets, int levelsup, int32_t *word, int32_t *node,
                   int32_t *bow_words, double *bow_values, int32_t *n_words, int32_t *fv_nodes, int32_t *fv_offsets, int32_t *fv_features,
                   int32_t *n_fv_nodes) {
    if (!voc) throw std::invalid_argument("null argument");
    if (n_sets < 0 || n_sets > (1 << 16)) throw std::invalid_argument("set count out of range");
    if (levelsup < 0) throw std::invalid_argument("levelsup is negative");
    if (n_sets == 0) return SIVO_OK;
    if (!offsets || !n_words || !fv_offsets || !n_fv_nodes) throw std::invalid_argument("null argument");
    if (offsets[0] != 0) throw std::invalid_argument("the offsets do not start at 0");
    int n_max = 0;
    for (int s = 0; s < n_sets; ++s) {
        const int64_t n = offsets[s + 1] - offsets[s];
        if (n < 0) throw std::invalid_argument("the offsets decrease");
        if (n > BOW_SET_CAP) throw std::invalid_argument("a set holds more than 8192 features");
        n_max = std::max(n_max, (int)n);
    }
    const int64_t total = offsets[n_sets];
    if (total > (int64_t)1 << 27) throw std::invalid_argument("batch too large");        // (the kernels index features in 32 bits)
    if (total > 0 && (!desc || !word || !node || !bow_words || !bow_values || !fv_nodes || !fv_features))
        throw std::invalid_argument("null argument");
    if (total == 0) {
        for (int s = 0; s < n_sets; ++s) { n_words[s] = 0; n_fv_nodes[s] = 0; fv_offsets[s] = 0; }
        return SIVO_OK;
    }
    require_device();
    static thread_local SolverCtx c(true, 512 << 10, 0, 1 << 20);
    c.bind();
    BowArgs a;
    a.v = bow_voc_on_device(voc);
    a.total = (int32_t)total; a.levelsup = levelsup;
    a.npad_max = 1;
    while (a.npad_max < n_max) a.npad_max <<= 1;
    const size_t T = (size_t)total, S = (size_t)n_sets;
    Layout L;
    L.copy(a.desc, desc, 32 * T);
    L.copy(a.sets, nullptr, sizeof(BowSetDesc) * S);
    L.take(a.bow_values, 8 * T); L.take(a.word, 4 * T); L.take(a.node, 4 * T); L.take(a.bow_words, 4 * T); L.take(a.n_words, 4 * S);
    L.take(a.fv_nodes, 4 * T); L.take(a.fv_off, 4 * (T + S)); L.take(a.fv_feat, 4 * T); L.take(a.n_fv, 4 * S);
#ifdef SIVO_DIAG
    L.take(a.stamps, 16 * S);
#endif
    L.take(a.leaf, 4 * T);                                           // (device scratch: last, outside the copy down)
    L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
    BowSetDesc *hs = L.host(a.sets);
    for (int s = 0; s < n_sets; ++s) hs[s] = BowSetDesc{offsets[s], (int32_t)(offsets[s + 1] - offsets[s]), 0};
    const size_t lds = 16 * (size_t)a.npad_max;
    static int attr_set[64];
    if (lds > (48u << 10))
        if (FirstUse once(attr_set); once)
            SIVO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(bow_set_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 16 * BOW_SET_CAP));
    L.send(c.stream);
    hipLaunchKernelGGL(bow_descend_kernel, dim3((unsigned)cdiv64(total * BOW_GROUP, BOW_THREADS)), dim3(BOW_THREADS), 0, c.stream, a);
    SIVO_HIP(hipGetLastError());
    hipLaunchKernelGGL(bow_set_kernel, dim3((unsigned)n_sets), dim3(BOW_THREADS), lds, c.stream, a);
    SIVO_HIP(hipGetLastError());
    const size_t down = (size_t)((const char *)a.leaf - (const char *)a.bow_values);
    SIVO_HIP(hipMemcpyAsync(L.host(a.bow_values), a.bow_values, down, hipMemcpyDeviceToHost, c.stream));
    SIVO_HIP(hipStreamSynchronize(c.stream));
    std::memcpy(bow_values, L.host(a.bow_values), 8 * T);
    std::memcpy(word, L.host(a.word), 4 * T);
    std::memcpy(node, L.host(a.node), 4 * T);
    std::memcpy(n_words, L.host(a.n_words), 4 * S);
    std::memcpy(n_fv_nodes, L.host(a.n_fv), 4 * S);
    const int32_t *hw = L.host(a.bow_words), *hn = L.host(a.fv_nodes), *ho = L.host(a.fv_off), *hf = L.host(a.fv_feat);
    for (int s = 0; s < n_sets; ++s) {                                // only what the counts say was written
        const size_t o = (size_t)offsets[s];
        const int nw = n_words[s], nf = n_fv_nodes[s];
        std::memcpy(bow_words + o, hw + o, 4 * (size_t)nw);
        std::memcpy(fv_nodes + o, hn + o, 4 * (size_t)nf);
        std::memcpy(fv_offsets + o + s, ho + o + s, 4 * ((size_t)nf + 1));
        std::memcpy(fv_features + o, hf + o, 4 * (size_t)ho[o + s + nf]);
    }
#ifdef SIVO_DIAG
    static int rate_khz[64];                                          // wall_clock64 ticks per millisecond, asked once per device
    int dev = 0;
    SIVO_HIP(hipGetDevice(&dev));
    int &rate = rate_khz[dev & 63];
    if (!rate) SIVO_HIP(hipDeviceGetAttribute(&rate, hipDeviceAttributeWallClockRate, dev));
    const int64_t *st = L.host(a.stamps);
    bow_last_set_us = rate > 0 ? 1e3 * (double)st[0] / rate : 0.0;
    bow_last_norm_us = rate > 0 ? 1e3 * (double)st[1] / rate : 0.0;
#endif
    return SIVO_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the keyframe database
// ---------------------------------------------------------------------------------------------------------------------
struct BowSlot { int64_t off; int32_t n, live; };

struct QueryArgs {
    const BowSlot *slots;
    const int32_t *words;
    const double *values;
    const int32_t *qw;
    const double *qv;
    int32_t n_slots, nq;
    int32_t *common, *first;
    double *score;
};

__global__ __launch_bounds__(BOW_THREADS) void bow_query_kernel(QueryArgs a) {
    extern __shared__ int32_t bow_q[];
    for (int i = (int)threadIdx.x; i < a.nq; i += BOW_THREADS) bow_q[i] = a.qw[i];
    __syncthreads();
    const int lane = (int)threadIdx.x & 63;
    const int slot = (int)blockIdx.x * BOW_QUERY_WAVES + ((int)threadIdx.x >> 6);
    if (slot >= a.n_slots) return;
    const BowSlot s = a.slots[slot];
    double sum = 0.0;
    int32_t common = 0, first = -1;
    for (int base = 0; base < s.n; base += 64) {
        const int j = base + lane;
        int32_t w = -1;
        int at = -1;
        if (j < s.n) {
            w = a.words[s.off + j];
            at = bow_find(bow_q, a.nq, w);
        }
        const double term = at >= 0 ? bow_l1_term(a.qv[at], a.values[s.off + j]) : 0.0;
        unsigned long long mask = __ballot(at >= 0);
        if (mask && first < 0) first = __shfl(w, __ffsll((long long)mask) - 1);
        common += __popcll(mask);
        while (mask) {                                              // the shared words of this chunk, ascending
            sum += __shfl(term, __ffsll((long long)mask) - 1);
            mask &= mask - 1;
        }
    }
    if (lane == 0) {
        a.common[slot] = common;
        a.first[slot] = first;
        a.score[slot] = bow_l1_finish(sum);
    }
}

}  // namespace sivo

using namespace sivo;

// The stored vectors in one grow-only slab (words, values) and a slot table, all on the device of the first add.
struct sivo_bowdb {
    int n_words = 0;                    // of the vocabulary: the bound of a word id
    std::mutex mutex;
    int device = -1;
    int32_t *d_words = nullptr;
    double *d_values = nullptr;
    BowSlot *d_slots = nullptr;
    int64_t cap_words = 0, used = 0;
    int32_t cap_slots = 0;
    std::vector<BowSlot> slots;
    SolverCtx ctx{true, 128 << 10, 0, 128 << 10};
    void release() {
        if (device < 0) return;
        DeviceRestore keep;
        if (hipSetDevice(device) != hipSuccess) return;
        (void)hipFree(d_words); (void)hipFree(d_values); (void)hipFree(d_slots);
        d_words = nullptr; d_values = nullptr; d_slots = nullptr;
    }
    void bind() {
        int d = 0;
        SIVO_HIP(hipGetDevice(&d));
        if (device < 0) device = d;
        if (device != d) throw std::invalid_argument("keyframe database: it lives on another device than the current one");
        ctx.bind();
    }
    template <class T>
    void grow(T *&p, int64_t old_count, int64_t new_cap) {
        T *q = nullptr;
        SIVO_HIP(hipMalloc((void **)&q, (size_t)new_cap * sizeof(T)));
        if (old_count) {
            const hipError_t e = hipMemcpyAsync(q, p, (size_t)old_count * sizeof(T), hipMemcpyDeviceToDevice, ctx.stream);
            const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(ctx.stream) : e;
            if (e2 != hipSuccess) { (void)hipFree(q); SIVO_HIP(e2); }
        }
        (void)hipFree(p);
        p = q;
    }
};

extern "C" int sivo_bow_transform_batch(sivo_voc_t voc, const uint8_t *desc, const int64_t *offsets, int n_sets, int levelsup, int32_t *word,
                                        int32_t *node, int32_t *bow_words, double *bow_values, int32_t *n_words, int32_t *fv_nodes,
                                        int32_t *fv_offsets, int32_t *fv_features, int32_t *n_fv_nodes) {
    return guarded([&] {
        return bow_run(voc, desc, offsets, n_sets, levelsup, word, node, bow_words, bow_values, n_words, fv_nodes, fv_offsets, fv_features,
                       n_fv_nodes);
    });
}

extern "C" int sivo_bow_transform(sivo_voc_t voc, const uint8_t *desc, int n, int levelsup, int32_t *word, int32_t *node, int32_t *bow_words,
                                  double *bow_values, int32_t *n_words, int32_t *fv_nodes, int32_t *fv_offsets, int32_t *fv_features,
                                  int32_t *n_fv_nodes) {
    return guarded([&] {
        if (n < 0) throw std::invalid_argument("feature count is negative");
        const int64_t offsets[2] = {0, n};
        return bow_run(voc, desc, offsets, 1, levelsup, word, node, bow_words, bow_values, n_words, fv_nodes, fv_offsets, fv_features, n_fv_nodes);
    });
}

#ifdef SIVO_DIAG
// Diagnostic build only (tools/bow_probe.py): the last sivo_bow_transform* call of this thread — microseconds the per-set kernel spent
// on its first set, and inside it on the ordered L1 norm, by the device's wall clock.
extern "C" int sivo_diag_bow_profile_read(double *set_us, double *norm_us) {
    if (set_us) *set_us = bow_last_set_us;
    if (norm_us) *norm_us = bow_last_norm_us;
    return SIVO_OK;
}
#endif

extern "C" int sivo_bowdb_create(sivo_voc_t voc, sivo_bowdb_t *db) {
    return guarded([&] {
        if (!voc || !db) throw std::invalid_argument("null argument");
        *db = new sivo_bowdb;
        (*db)->n_words = voc->img.n_words;
        return SIVO_OK;
    });
}

extern "C" int sivo_bowdb_destroy(sivo_bowdb_t db) {
    return guarded([&] {
        if (!db) return SIVO_OK;
        db->release();
        delete db;
        return SIVO_OK;
    });
}

extern "C" int sivo_bowdb_size(sivo_bowdb_t db, int32_t *n_slots) {
    return guarded([&] {
        if (!db || !n_slots) throw std::invalid_argument("null argument");
        std::lock_guard<std::mutex> lock(db->mutex);
        *n_slots = (int32_t)db->slots.size();
        return SIVO_OK;
    });
}

extern "C" int sivo_bowdb_add(sivo_bowdb_t db, const int32_t *words, const double *values, int n, int32_t *slot) {
    return guarded([&] {
        if (!db || !slot) throw std::invalid_argument("null argument");
        bow_check_vector(words, values, n, db->n_words);
        std::lock_guard<std::mutex> lock(db->mutex);
        if (db->slots.size() >= (size_t)1 << 24) throw std::invalid_argument("keyframe database: too many slots");
        require_device();
        db->bind();
        const int32_t id = (int32_t)db->slots.size();
        if (db->used + n > db->cap_words) {
            const int64_t cap = std::max<int64_t>(2 * (db->used + n), 1 << 16);
            db->grow(db->d_words, db->used, cap);
            db->grow(db->d_values, db->used, cap);
            db->cap_words = cap;
        }
        if (id + 1 > db->cap_slots) {
            const int32_t cap = std::max(2 * (id + 1), 1024);
            db->grow(db->d_slots, (int64_t)id, (int64_t)cap);
            db->cap_slots = cap;
        }
        const BowSlot rec{db->used, n, 1};
        hipStream_t st = db->ctx.stream;
        if (n) {
            SIVO_HIP(hipMemcpyAsync(db->d_words + db->used, words, 4 * (size_t)n, hipMemcpyHostToDevice, st));
            SIVO_HIP(hipMemcpyAsync(db->d_values + db->used, values, 8 * (size_t)n, hipMemcpyHostToDevice, st));
        }
        SIVO_HIP(hipMemcpyAsync(db->d_slots + id, &rec, sizeof rec, hipMemcpyHostToDevice, st));
        SIVO_HIP(hipStreamSynchronize(st));
        db->slots.push_back(rec);
        db->used += n;
        *slot = id;
        return SIVO_OK;
    });
}

extern "C" int sivo_bowdb_erase(sivo_bowdb_t db, int32_t slot) {
    return guarded([&] {
        if (!db) throw std::invalid_argument("null argument");
        std::lock_guard<std::mutex> lock(db->mutex);
        if (slot < 0 || (size_t)slot >= db->slots.size() || !db->slots[(size_t)slot].live)
            throw std::invalid_argument("keyframe database: no such slot");
        db->bind();
        const BowSlot rec{db->slots[(size_t)slot].off, 0, 0};          // a tombstone: no words
        SIVO_HIP(hipMemcpyAsync(db->d_slots + slot, &rec, sizeof rec, hipMemcpyHostToDevice, db->ctx.stream));
        SIVO_HIP(hipStreamSynchronize(db->ctx.stream));
        db->slots[(size_t)slot] = rec;
        return SIVO_OK;
    });
}

extern "C" int sivo_bowdb_clear(sivo_bowdb_t db) {
    return guarded([&] {
        if (!db) throw std::invalid_argument("null argument");
        std::lock_guard<std::mutex> lock(db->mutex);
        db->slots.clear();
        db->used = 0;
        return SIVO_OK;
    });
}

extern "C" int sivo_bowdb_query(sivo_bowdb_t db, const int32_t *q_words, const double *q_values, int nq, int32_t *common, int32_t *first_word,
                                double *score, int32_t *n_slots) {
    return guarded([&] {
        if (!db || !n_slots) throw std::invalid_argument("null argument");
        bow_check_vector(q_words, q_values, nq, db->n_words);
        std::lock_guard<std::mutex> lock(db->mutex);
        const int32_t n = (int32_t)db->slots.size();
        *n_slots = n;
        if (n == 0) return SIVO_OK;
        if (!common || !first_word || !score) throw std::invalid_argument("null argument");
        require_device();
        db->bind();
        SolverCtx &c = db->ctx;
        QueryArgs a;
        a.slots = db->d_slots; a.words = db->d_words; a.values = db->d_values;
        a.n_slots = n; a.nq = nq;
        Layout L;
        L.copy(a.qw, q_words, 4 * (size_t)nq);
        L.copy(a.qv, q_values, 8 * (size_t)nq);
        L.take(a.score, 8 * (size_t)n); L.take(a.common, 4 * (size_t)n); L.take(a.first, 4 * (size_t)n);
        L.place(c.dev.reserve(L.bytes()), c.in.reserve(L.bytes()));
        L.send(c.stream);
        hipLaunchKernelGGL(bow_query_kernel, dim3((unsigned)cdiv(n, BOW_QUERY_WAVES)), dim3(BOW_THREADS), 4 * (size_t)std::max(nq, 1), c.stream, a);
        SIVO_HIP(hipGetLastError());
        SIVO_HIP(hipMemcpyAsync(L.host(a.score), a.score, L.results(), hipMemcpyDeviceToHost, c.stream));
        SIVO_HIP(hipStreamSynchronize(c.stream));
        std::memcpy(score, L.host(a.score), 8 * (size_t)n);
        std::memcpy(common, L.host(a.common), 4 * (size_t)n);
        std::memcpy(first_word, L.host(a.first), 4 * (size_t)n);
        return SIVO_OK;
    });
}
