// ba_sparse_plan.hpp — what the host prepares once per BaSolver for the sparse reduced camera system (ba_solve.hip): the
// pattern of S (a block (i, j) of free poses exists when the two share a point, whatever the edges' level), its ordering and symbolic
// factorisation (sparse_plan.hpp) and, per owner block, the list of (edge of the row pose, edge of the column pose) pairs through the
// same point in increasing point order.  Host only, the standard library alone: the stand-alone test programs compile it with g++.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../include/sivo_hip.h"
#include "sparse_plan.hpp"

namespace sivo {

// AUTO takes the sparse path from this many free keyframes on (and whenever the dense path would refuse the problem).  Never below 64:
// every problem of at most 30 keyframes stays on the dense path, bit for bit.  64 is also the measured crossover, the smallest rung from
// 64 up at which the whole sparse call is faster (MI355X, tools/ba_sparse_probe.py, ms per ba_optimize(..., 1) call, dense / sparse):
//   32 free keyframes 0.857 / 0.603    64: 3.730 / 1.058    128: 24.53 / 1.886    256: 185.8 / 3.599    512: 1458.3 / 7.211
//   sparse only: 1024: 13.41    2048: 30.16 (host plan 10.1 ms of it, factor + solve kernel 18.7 ms)            DESIGN 3.6l has the table.
constexpr int BA_SPARSE_MIN_FREE = 64;
constexpr int64_t BA_DENSE_TABLE_MAX = (int64_t)1 << 28;

// the path a solver option takes: 1 dense, 2 sparse
inline int ba_choose_path(int solver, int nF, int64_t nX) {
    if (solver < SIVO_BA_SOLVER_AUTO || solver > SIVO_BA_SOLVER_SPARSE) throw std::invalid_argument("SivoBaOptions.solver must be 0 (auto), 1 (dense) or 2 (sparse)");
    const bool refused = (int64_t)nF * nX > BA_DENSE_TABLE_MAX;
    if (solver == SIVO_BA_SOLVER_SPARSE) return 2;
    if (solver == SIVO_BA_SOLVER_DENSE) {
        if (refused) throw std::invalid_argument("problem too large for the dense (free pose x point) edge table");
        return 1;
    }
    return refused || nF >= BA_SPARSE_MIN_FREE ? 2 : 1;
}
inline int ba_solver_option(const SivoBaOptions *o) {
    if (!o) return SIVO_BA_SOLVER_AUTO;
    if (o->size < sizeof(uint32_t) + sizeof(int32_t)) throw std::invalid_argument("SivoBaOptions.size is smaller than the structure's first version");
    return o->solver;
}

struct BaSparsePlan {
    SparsePattern pat;                          // variables = free slots
    std::vector<int32_t> perm;                  // elimination position -> free slot
    std::vector<int32_t> own_blk, con_ptr, con; // owner blocks (every diagonal block, then the off-diagonal blocks of S): L block id, CSR of (edge, edge) pairs
    int64_t n_pairs = 0;                        // contribution pairs in all
    int n_off = 0;                              // blocks of S below the diagonal
    int64_t nnzL = 0, flops = 0;
};

// pt_off / pt_edges: the edges by point (CSR, edge order within a point); slot: pose -> free slot or -1
inline void ba_sparse_plan(const SivoEdge *edges, const int32_t *slot, int nF, int nX, const int64_t *pt_off, const int32_t *pt_edges,
                           BaSparsePlan &P) {
    // the free observers of every point, by slot; two edges on one (keyframe, point) pair are refused as the dense table refuses them
    std::vector<int64_t> ob_off((size_t)nX + 1, 0);
    std::vector<std::pair<int32_t, int32_t>> ob;            // (slot, edge)
    int64_t total = 0;
    for (int q = 0; q < nX; ++q) {
        const size_t first = ob.size();
        for (int64_t i = pt_off[q]; i < pt_off[q + 1]; ++i) {
            const int32_t e = pt_edges[i], s = slot[edges[e].pose];
            if (s >= 0) ob.push_back({s, e});
        }
        std::sort(ob.begin() + first, ob.end());
        for (size_t i = first + 1; i < ob.size(); ++i)
            if (ob[i].first == ob[i - 1].first) throw std::invalid_argument("two edges join the same (keyframe, map point) pair");
        const int64_t k = (int64_t)(ob.size() - first);
        total += k * (k + 1) / 2;
        if (total > (int64_t)INT32_MAX)
            throw std::invalid_argument("the contribution lists of the sparse reduced system would exceed 2^31 - 1 entries");
        ob_off[q + 1] = (int64_t)ob.size();
    }
    P.n_pairs = total;
    // the pattern: every pair of free poses with a common point (compacted now and then: a point of k observers names k (k - 1) / 2 pairs)
    std::vector<std::pair<int, int>> vp;
    auto compact = [&] { std::sort(vp.begin(), vp.end()); vp.erase(std::unique(vp.begin(), vp.end()), vp.end()); };
    size_t next_compact = (size_t)1 << 22;
    for (int q = 0; q < nX; ++q) {
        for (int64_t a = ob_off[q]; a < ob_off[q + 1]; ++a)
            for (int64_t b = a + 1; b < ob_off[q + 1]; ++b) vp.push_back({ob[a].first, ob[b].first});
        if (vp.size() > next_compact) { compact(); next_compact = std::max(next_compact, 2 * vp.size()); }
    }
    compact();
    SparsePattern &pat = P.pat;
    sparse_pattern(nF, vp, pat);
    const int na = nF, nL = pat.nL;
    P.perm.assign((size_t)na, 0);
    for (int s = 0; s < na; ++s) P.perm[pat.pos[s]] = s;
    // owners and their lists: count, then fill in point order (row = the pose eliminated later)
    std::vector<int32_t> cnt((size_t)std::max(nL, 1), 0);
    auto block_of = [&](int pa, int pb) { return pa == pb ? pa : pa > pb ? pat.find_blk(pa, pb) : pat.find_blk(pb, pa); };
    for (int q = 0; q < nX; ++q)
        for (int64_t a = ob_off[q]; a < ob_off[q + 1]; ++a)
            for (int64_t b = a; b < ob_off[q + 1]; ++b) cnt[block_of(pat.pos[ob[a].first], pat.pos[ob[b].first])]++;
    std::vector<int32_t> owner((size_t)std::max(nL, 1), -1);
    P.con_ptr.push_back(0);
    for (int b = 0; b < nL; ++b) {
        if (b >= na && cnt[b] == 0) continue;                 // (a fill block: nothing of S in it)
        owner[b] = (int32_t)P.own_blk.size();
        P.own_blk.push_back(b);
        P.con_ptr.push_back(P.con_ptr.back() + cnt[b]);
        if (b >= na) ++P.n_off;
    }
    P.con.assign(2 * (size_t)total + 2, 0);
    std::vector<int32_t> fill(P.con_ptr.begin(), P.con_ptr.end() - 1);
    for (int q = 0; q < nX; ++q)
        for (int64_t a = ob_off[q]; a < ob_off[q + 1]; ++a)
            for (int64_t b = a; b < ob_off[q + 1]; ++b) {
                const int pa = pat.pos[ob[a].first], pb = pat.pos[ob[b].first];
                const size_t at = 2 * (size_t)fill[owner[block_of(pa, pb)]]++;
                P.con[at] = pa >= pb ? ob[a].second : ob[b].second;
                P.con[at + 1] = pa >= pb ? ob[b].second : ob[a].second;
            }
    // nnz(L) (lower triangle, scalars) and the flops of one numeric factorisation: 2 x 216 per block product, 112 per 6 x 6 Cholesky
    // (6^3 / 3 and the reciprocals), 216 per panel solve
    P.nnzL = 21 * (int64_t)na + 36 * (int64_t)(nL - na);
    P.flops = 432 * (int64_t)(pat.pairs.size() / 2) + 112 * (int64_t)na + 216 * (int64_t)(nL - na);
}

// The checks of BaSolver's constructor that need no device, the CSR by point and, when asked for, by free pose (edge order within a
// list): two passes over the edges.  Shared with sivo_ba_analyze.
inline void ba_index_edges(const uint8_t *fixed, int nP, int nX, const SivoEdge *edges, int64_t nE, std::vector<int32_t> &slot, int &nF,
                           std::vector<int64_t> &pt_off, std::vector<int32_t> &pt_edges, std::vector<int64_t> *ps_off = nullptr,
                           std::vector<int32_t> *ps_edges = nullptr) {
    if (nP < 0 || nX < 0 || nE < 0) throw std::invalid_argument("negative size");
    if (nE > INT32_MAX) throw std::invalid_argument("too many edges");
    slot.assign((size_t)std::max(nP, 1), -1);
    nF = 0;
    for (int i = 0; i < nP; ++i) slot[i] = fixed && fixed[i] ? -1 : nF++;
    pt_off.assign((size_t)nX + 1, 0);
    if (ps_off) ps_off->assign((size_t)nF + 1, 0);
    for (int64_t e = 0; e < nE; ++e) {
        if (edges[e].pose < 0 || edges[e].pose >= nP || edges[e].point < 0 || edges[e].point >= nX)
            throw std::invalid_argument("edge refers to a pose/point outside the arrays");
        pt_off[edges[e].point + 1]++;
        if (ps_off && slot[edges[e].pose] >= 0) (*ps_off)[slot[edges[e].pose] + 1]++;
    }
    for (int q = 0; q < nX; ++q) pt_off[q + 1] += pt_off[q];
    pt_edges.assign((size_t)std::max<int64_t>(nE, 1), 0);
    std::vector<int64_t> f1(pt_off.begin(), pt_off.end() - 1), f2;
    if (ps_off) {
        for (int s = 0; s < nF; ++s) (*ps_off)[s + 1] += (*ps_off)[s];
        ps_edges->assign((size_t)std::max<int64_t>((*ps_off)[nF], 1), 0);
        f2.assign(ps_off->begin(), ps_off->end() - 1);
    }
    for (int64_t e = 0; e < nE; ++e) {
        pt_edges[f1[edges[e].point]++] = (int32_t)e;
        if (ps_off && slot[edges[e].pose] >= 0) (*ps_edges)[f2[slot[edges[e].pose]]++] = (int32_t)e;
    }
}

}  // namespace sivo
