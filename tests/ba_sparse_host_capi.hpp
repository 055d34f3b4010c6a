// ba_sparse_host_capi.hpp — the sparse path of the bundle adjustment's reduced camera system on the host: the plan of
// sivo_amd/csrc/ba_sparse_plan.hpp and a sequential walk over its blocks through the per-block bodies of sivo_amd/csrc/ba_sparse_math.hpp,
// the same code and the same order of every sum as ba_sparse_schur_kernel / ba_sparse_solve_kernel (ba_solve.hip), where one lane has
// one entry of a block.  For tests/ba_sparse_prog.cpp; C++14, no device.
#pragma once
#include <cstdint>
#include <vector>

#include "ba_sparse_math.hpp"
#include "ba_sparse_plan.hpp"

namespace ba_sparse_host {

struct Problem {
    int nP = 0, nX = 0;
    int64_t nE = 0;
    double lambda = 0.0;
    std::vector<uint8_t> fixed, level;
    std::vector<SivoEdge> edges;
    std::vector<double> W, Hll, bl, Hpp, bp;      // 18 per edge, 9 and 3 per point, 36 and 6 per free slot
};

struct Result {
    int nF = 0, ok = 0;
    sivo::BaSparsePlan plan;
    std::vector<int32_t> own_rc;                  // per owner: the free slots of its row and column
    std::vector<double> S, rhs, x;                // 36 per owner; 6 per free slot; 6 per free slot (zero when ok = 0)
};

inline void solve(const Problem &p, Result &R) {
    using namespace sivo;
    std::vector<int32_t> slot, pt_edges;
    std::vector<int64_t> pt_off;
    ba_index_edges(p.fixed.data(), p.nP, p.nX, p.edges.data(), p.nE, slot, R.nF, pt_off, pt_edges);
    BaSparsePlan &P = R.plan;
    ba_sparse_plan(p.edges.data(), slot.data(), R.nF, p.nX, pt_off.data(), pt_edges.data(), P);
    const SparsePattern &pat = P.pat;
    const int na = R.nF, nL = pat.nL, n_own = (int)P.own_blk.size();
    std::vector<double> H((size_t)nL * 36, 0.0), b((size_t)na * 6, 0.0), L((size_t)nL * 36, 0.0), rinv((size_t)na * 6, 0.0), x((size_t)na * 6, 0.0);
    // S, owner by owner (ba_sparse_schur_kernel): lanes 0 .. 35 the entries, 36 .. 41 the right-hand side of a diagonal owner
    for (int o = 0; o < n_own; ++o) {
        const int blk = P.own_blk[o];
        const bool diag = blk < na;
        for (int lane = 0; lane < 42; ++lane) {
            const bool ent = lane < 36, rhs = diag && lane >= 36;
            if (!ent && !rhs) continue;
            const int r = ent ? lane / 6 : lane - 36, c = ent ? lane % 6 : 0;
            double acc = 0.0;
            for (int64_t q = P.con_ptr[o]; q < P.con_ptr[o + 1]; ++q) {
                const int e1 = P.con[2 * q], e2 = P.con[2 * q + 1];
                if (p.level[e1] || p.level[e2]) continue;
                const int pt = p.edges[e1].point;
                double Ai[9], y[3];
                bs_point_inverse(p.Hll.data() + 9 * (int64_t)pt, p.lambda, Ai);
                bs_y_row(p.W.data() + 18 * (int64_t)e1 + 3 * r, Ai, y);
                acc += bs_contrib(y, rhs ? p.bl.data() + 3 * (int64_t)pt : p.W.data() + 18 * (int64_t)e2 + 3 * c);
            }
            if (ent) {
                double v = -acc;
                if (diag) { v += p.Hpp[36 * (int64_t)P.perm[blk] + lane]; if (r == c) v += p.lambda; }
                H[(int64_t)blk * 36 + lane] = v;
            } else {
                b[(int64_t)blk * 6 + r] = p.bp[6 * (int64_t)P.perm[blk] + r] - acc;
            }
        }
        R.own_rc.push_back(P.perm[pat.blk_row[blk]]);
        R.own_rc.push_back(P.perm[pat.blk_col[blk]]);
        R.S.insert(R.S.end(), H.begin() + (int64_t)blk * 36, H.begin() + (int64_t)blk * 36 + 36);
    }
    R.rhs.assign((size_t)na * 6, 0.0);
    for (int j = 0; j < na; ++j)
        for (int m = 0; m < 6; ++m) R.rhs[6 * (size_t)P.perm[j] + m] = b[6 * (size_t)j + m];
    // factorisation, level by level (ba_sparse_solve_kernel)
    auto pair_sum = [&](int blk, int r, int c) {
        double acc = 0.0;
        for (int q = pat.pair_ptr[blk]; q < pat.pair_ptr[blk + 1]; ++q)
            acc += bs_dot6(L.data() + (int64_t)pat.pairs[2 * (int64_t)q] * 36 + 6 * r, L.data() + (int64_t)pat.pairs[2 * (int64_t)q + 1] * 36 + 6 * c);
        return acc;
    };
    bool ok = true;
    for (int lv = 0; lv < pat.nlev; ++lv) {
        for (int t = pat.lvl_ptr[lv]; t < pat.lvl_ptr[lv + 1]; ++t) {
            const int j = pat.lvl_col[t];
            double A[36], rd[6];
            for (int k = 0; k < 36; ++k) A[k] = H[(int64_t)j * 36 + k] - pair_sum(j, k / 6, k % 6);
            if (!bs_chol6(A, rd)) ok = false;
            for (int k = 0; k < 36; ++k) L[(int64_t)j * 36 + k] = k % 6 <= k / 6 ? A[k] : 0.0;
            for (int k = 0; k < 6; ++k) rinv[(int64_t)j * 6 + k] = rd[k];
        }
        for (int t = pat.off_ptr[lv]; t < pat.off_ptr[lv + 1]; ++t) {
            const int blk = pat.off_blk[t], j = pat.blk_col[blk];
            for (int r = 0; r < 6; ++r) {
                double row[6], X[6];
                for (int m = 0; m < 6; ++m) row[m] = H[(int64_t)blk * 36 + 6 * r + m] - pair_sum(blk, r, m);
                bs_panel_row(row, L.data() + (int64_t)j * 36, rinv.data() + (int64_t)j * 6, X);
                for (int m = 0; m < 6; ++m) L[(int64_t)blk * 36 + 6 * r + m] = X[m];
            }
        }
    }
    R.ok = ok ? 1 : 0;
    R.x.assign((size_t)na * 6, 0.0);
    if (!ok) return;
    for (int lv = 0; lv < pat.nlev; ++lv)
        for (int t = pat.lvl_ptr[lv]; t < pat.lvl_ptr[lv + 1]; ++t) {
            const int j = pat.lvl_col[t];
            double sv[6], y[6];
            for (int rr = 0; rr < 6; ++rr) {
                double a = b[(int64_t)j * 6 + rr];
                for (int q = pat.row_ptr[j]; q < pat.row_ptr[j + 1]; ++q)
                    a -= bs_dot6(L.data() + (int64_t)pat.row_lst[2 * q] * 36 + 6 * rr, x.data() + (int64_t)pat.row_lst[2 * q + 1] * 6);
                sv[rr] = a;
            }
            bs_forward6(sv, L.data() + (int64_t)j * 36, rinv.data() + (int64_t)j * 6, y);
            for (int m = 0; m < 6; ++m) x[(int64_t)j * 6 + m] = y[m];
        }
    for (int lv = pat.nlev - 1; lv >= 0; --lv)
        for (int t = pat.lvl_ptr[lv]; t < pat.lvl_ptr[lv + 1]; ++t) {
            const int j = pat.lvl_col[t];
            double sv[6], xx[6];
            for (int rr = 0; rr < 6; ++rr) {
                double a = x[(int64_t)j * 6 + rr];
                for (int q = pat.col_ptr[j]; q < pat.col_ptr[j + 1]; ++q)
                    a -= bs_dot6_col(L.data() + (int64_t)pat.col_lst[2 * q] * 36 + rr, x.data() + (int64_t)pat.col_lst[2 * q + 1] * 6);
                sv[rr] = a;
            }
            bs_backward6(sv, L.data() + (int64_t)j * 36, rinv.data() + (int64_t)j * 6, xx);
            for (int m = 0; m < 6; ++m) { x[(int64_t)j * 6 + m] = xx[m]; R.x[6 * (size_t)P.perm[j] + m] = xx[m]; }
        }
}

}  // namespace ba_sparse_host
