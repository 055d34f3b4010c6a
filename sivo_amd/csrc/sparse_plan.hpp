// sparse_plan.hpp — ordering and symbolic block Cholesky of a sparse symmetric block system, host only (the standard library alone: the
// stand-alone test programs compile it with g++).  Shared by the Sim3 pose graph (essential_graph.hip: 7 x 7 blocks) and the sparse reduced
// camera system of the bundle adjustment (ba_solve.hip: 6 x 6 blocks).  The caller names its variables 0 .. na - 1 and lists the pairs of
// variables that share an off-diagonal block; everything here is about the pattern, nothing about block sizes or values.
#pragma once
#include <algorithm>
#include <cstdint>
#include <iterator>
#include <stdexcept>
#include <utility>
#include <vector>

namespace sivo {

struct SparsePattern {
    int na = 0, nlev = 0, nL = 0;               // variables, levels of the elimination tree, blocks of L (diagonal ones included)
    std::vector<int> pos;                       // variable -> elimination position
    std::vector<int> lvl_ptr, lvl_col;          // levels of the elimination tree: positions per level
    std::vector<int> off_ptr, off_blk;          // the off-diagonal L blocks of each level's columns
    std::vector<int> blk_col, blk_row;          // per L block: its column / row (diagonal blocks: the position)
    std::vector<int> pair_ptr, pairs;           // per L block: the (L_ik, L_jk) block pairs its update sums (diagonal: L_jk twice)
    std::vector<int> row_ptr, row_lst;          // per position j: the blocks (j, k < j) of L, with k: 2 ints each
    std::vector<int> col_ptr, col_lst;          // per position j: the blocks (i > j, j) of L, with i: 2 ints each
    std::vector<std::vector<int>> colrows, colblk;      // per column: the rows of its off-diagonal blocks (ascending) and their block ids
    int find_blk(int i, int j) const {          // the L block (i > j, j)
        const auto &cr = colrows[j];
        const size_t q = std::lower_bound(cr.begin(), cr.end(), i) - cr.begin();
        return colblk[j][q];
    }
};

// Minimum degree on the block graph with the explicit elimination graph (ties to the lower variable), the blocks of L, the per-block
// update lists and the levels of the elimination tree.  `var_pairs` may name a pair more than once and in either order.
inline void sparse_pattern(int na, const std::vector<std::pair<int, int>> &var_pairs, SparsePattern &P) {
    P.na = na;
    if (na == 0) return;
    std::vector<std::vector<int>> adj(na);
    for (const auto &ab : var_pairs) { adj[ab.first].push_back(ab.second); adj[ab.second].push_back(ab.first); }
    for (auto &l : adj) { std::sort(l.begin(), l.end()); l.erase(std::unique(l.begin(), l.end()), l.end()); }
    std::vector<int> &pos = P.pos;
    pos.assign(na, -1);
    std::vector<std::vector<int>> colv(na);   // per position: the variables of the column's pattern (eliminated later)
    std::vector<int> merged;
    for (int step = 0; step < na; ++step) {
        int best = -1;
        size_t bd = 0;
        for (int v = 0; v < na; ++v)
            if (pos[v] < 0 && (best < 0 || adj[v].size() < bd)) { best = v; bd = adj[v].size(); }
        pos[best] = step;
        colv[step] = adj[best];
        for (int u : adj[best]) {             // the neighbours become a clique, best leaves the graph
            merged.clear();
            std::set_union(adj[u].begin(), adj[u].end(), adj[best].begin(), adj[best].end(), std::back_inserter(merged));
            merged.erase(std::remove_if(merged.begin(), merged.end(), [&](int w) { return w == u || w == best; }), merged.end());
            adj[u].swap(merged);
        }
        adj[best].clear();
    }
    // the blocks of L: diagonal p = position p, then the off-diagonal ones column by column, rows ascending
    std::vector<std::vector<int>> &colrows = P.colrows, &colblk = P.colblk;
    colrows.assign(na, {}); colblk.assign(na, {});
    int64_t nL64 = na;
    for (int j = 0; j < na; ++j) nL64 += (int64_t)colv[j].size();
    if (nL64 > INT32_MAX / 64) throw std::invalid_argument("the factor of the sparse system has too many blocks");
    int nL = na;
    for (int j = 0; j < na; ++j) {
        for (int v : colv[j]) colrows[j].push_back(pos[v]);
        std::sort(colrows[j].begin(), colrows[j].end());
        for (size_t q = 0; q < colrows[j].size(); ++q) colblk[j].push_back(nL++);
    }
    P.nL = nL;
    P.blk_col.assign(nL, 0);
    P.blk_row.assign(nL, 0);
    for (int j = 0; j < na; ++j) { P.blk_col[j] = j; P.blk_row[j] = j; }
    for (int j = 0; j < na; ++j)
        for (size_t q = 0; q < colrows[j].size(); ++q) { P.blk_col[colblk[j][q]] = j; P.blk_row[colblk[j][q]] = colrows[j][q]; }
    // rows: per position i, the blocks (i, k < i) with k ascending
    std::vector<std::vector<std::pair<int, int>>> rows(na);      // (k, block)
    for (int j = 0; j < na; ++j)
        for (size_t q = 0; q < colrows[j].size(); ++q) rows[colrows[j][q]].push_back({j, colblk[j][q]});
    P.row_ptr.assign(na + 1, 0);
    for (int i = 0; i < na; ++i) {
        P.row_ptr[i + 1] = P.row_ptr[i] + (int)rows[i].size();
        for (auto &kb : rows[i]) { P.row_lst.push_back(kb.second); P.row_lst.push_back(kb.first); }
    }
    P.col_ptr.assign(na + 1, 0);
    for (int j = 0; j < na; ++j) {
        P.col_ptr[j + 1] = P.col_ptr[j] + (int)colrows[j].size();
        for (size_t q = 0; q < colrows[j].size(); ++q) { P.col_lst.push_back(colblk[j][q]); P.col_lst.push_back(colrows[j][q]); }
    }
    // the update lists: block (i, j) sums L_ik L_jk^T over k < j in both rows (k ascending); diagonal (j, j) over the whole row j
    P.pair_ptr.assign(nL + 1, 0);
    std::vector<int> bp;
    for (int b = 0; b < nL; ++b) {
        bp.clear();
        if (b < na) {
            for (auto &kb : rows[b]) { bp.push_back(kb.second); bp.push_back(kb.second); }
        } else {
            const auto &ri = rows[P.blk_row[b]], &rj = rows[P.blk_col[b]];
            size_t a = 0, c = 0;
            while (a < ri.size() && c < rj.size()) {
                if (ri[a].first < rj[c].first) ++a;
                else if (ri[a].first > rj[c].first) ++c;
                else { bp.push_back(ri[a].second); bp.push_back(rj[c].second); ++a; ++c; }
            }
        }
        if (P.pairs.size() + bp.size() > (size_t)INT32_MAX) throw std::invalid_argument("the update lists of the sparse factorisation are too long");
        P.pair_ptr[b + 1] = P.pair_ptr[b] + (int)bp.size() / 2;
        P.pairs.insert(P.pairs.end(), bp.begin(), bp.end());
    }
    // levels of the elimination tree (parent = first row of the column's pattern): a column sits one level above its highest child
    std::vector<int> level(na, 0);
    int nlev = 0;
    for (int j = 0; j < na; ++j) {
        nlev = std::max(nlev, level[j] + 1);
        if (!colrows[j].empty()) { const int p = colrows[j][0]; level[p] = std::max(level[p], level[j] + 1); }
    }
    P.nlev = nlev;
    P.lvl_ptr.assign(nlev + 1, 0);
    P.off_ptr.assign(nlev + 1, 0);
    std::vector<std::vector<int>> bylev(nlev);
    for (int j = 0; j < na; ++j) bylev[level[j]].push_back(j);
    for (int l = 0; l < nlev; ++l) {
        for (int j : bylev[l]) {
            P.lvl_col.push_back(j);
            for (int blk : colblk[j]) P.off_blk.push_back(blk);
        }
        P.lvl_ptr[l + 1] = (int)P.lvl_col.size();
        P.off_ptr[l + 1] = (int)P.off_blk.size();
    }
}

}  // namespace sivo
