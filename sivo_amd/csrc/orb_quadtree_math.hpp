// orb_quadtree_math.hpp — ORBextractor::DistributeOctTree (reference ORBextractor.cc:544-750) as rounds of data-parallel steps: the
// per-candidate and per-cell bodies and the driver that orders them.  orb_quadtree.hip runs them with one workgroup per candidate
// set (a body over n items = a strided loop and a barrier); tests/orb_quadtree_prog.cpp walks the same bodies one item after the
// other on the host.  The result equals distribute_quadtree (orb_host.cpp) byte for byte.
//
// Why a round is a parallel step.  A candidate is three small integers (x:12 | y:12 | response:8 in one word), a cell is an integer
// box, ceil((float)d / 2) is (d + 1) >> 1.  A cell's candidates are always a subsequence of the input in input order, so "arrival
// order" is index order: nothing is moved, a candidate only carries the list position of its cell, and "greatest response, first one
// wins" is "greatest response, then smallest index".  One pass of the reference's `while (!bFinish)` loop splits every non-leaf cell
// p1 .. pm of the list independently: the new list is the non-empty children of pm in the order SE, SW, NE, NW, then those of pm-1,
// ... p1, then the old leaves in their order; `grown` (the children with more than one candidate) in creation order is p1's NW, NE,
// SW, SE, then p2's, ...  One pass of the close-to-target phase sorts `grown` by (size, creation order) descending, counts the
// quadrants of all of them, takes the inclusive scan of (non-empty children - 1) on top of the list's count and stops at the first
// position J whose scan reaches the target (the last one if none does); positions 0 .. J are split, the children of J come first.
// Both are the same step here: an order `srt` of the cells that may split (list order / sorted order), a scan over it, a stop
// position J (the last / the first that reaches the target), a scan of the cells that stay, one write of the new list, one remap of
// the candidates.
//
// Bounds.  The list never holds more than max(target + 3, 4 * n_ini) cells (the first round splits at most the roots; a later full
// round is taken only when count + 3 * n_expand <= target; the close-to-target phase stops at the first count >= target); the caller
// refuses a set whose bound exceeds QT_MAX_CELLS, and the driver checks every new count against the table before it writes.  Cell
// extents halve per pass, a pass that changes nothing ends the loop (count == before, as on the host), and QT_MAX_ROUNDS caps the
// passes.  Exceeding a bound returns a status and no list.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QT_HD __host__ __device__
#else
#define QT_HD
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define QT_ADD(p, v) atomicAdd((p), (v))
#define QT_MAX(p, v) atomicMax((p), (v))
#define QT_MIN(p, v) atomicMin((p), (v))
#define QT_FDIV(a, b) __fdiv_rn((a), (b))
#define QT_FMUL(a, b) __fmul_rn((a), (b))
#else
#define QT_ADD(p, v) (*(p) += (v))
#define QT_MAX(p, v) (*(p) = *(p) < (v) ? (v) : *(p))
#define QT_MIN(p, v) (*(p) = *(p) > (v) ? (v) : *(p))
#define QT_FDIV(a, b) ((a) / (b))
#define QT_FMUL(a, b) ((a) * (b))
#endif

namespace sivo {

constexpr int QT_MAX_CELLS = 2048;        // cells of one set's list (the table of a workgroup)
constexpr int QT_MAX_ROUNDS = 64;         // passes of either kind (extents below 4096 allow about 26)
constexpr int QT_MAX_EXTENT = 4096;       // 12 bits per coordinate
constexpr uint16_t QT_NONE = 0xffff;
enum { QT_OK = 0, QT_ERR_CELLS = 1, QT_ERR_ROUNDS = 2, QT_ERR_OFFSETS = 3, QT_ERR_SLOTS = 4 };

struct QtCell { uint16_t x0, y0, x1, y1; int32_t n; };      // [x0, x1) x [y0, y1), candidates inside

// One candidate set.  off_b / off_e index the offset table the candidates' producer wrote (the set is words[off[off_b] .. off[off_e]));
// w, h: the region's extents; h_x = (float)w / n_ini and n_ini = round(w / h) come from the host, as the reference computes them;
// slot_base / slot_count: where the kept words go and how many fit.
struct QtSet { int32_t off_b, off_e, w, h, n_ini, target; float h_x; int32_t slot_base, slot_count; };

// max(target + 3, 4 * n_ini): what the list of a set can hold at most (see Bounds)
QT_HD inline int64_t qt_cell_bound(int target, int n_ini) {
    const int64_t a = (int64_t)target + 3, b = 4 * (int64_t)n_ini;
    return a > b ? a : b;
}

struct QtState {
    const uint32_t *word;     // n packed candidates
    uint16_t *cid;            // n: list position of the candidate's cell
    int n;
    QtCell *cur, *nxt;        // the list and the one being written (QT_MAX_CELLS each)
    int32_t (*cnt4)[4];       // per cell: candidates per quadrant NW, NE, SW, SE; after the write of the new list the new positions
    uint32_t *sc;             // scan over the split order: non-empty children | grown children << 16
    uint32_t *sk;             // scan over the list: cells that stay
    uint16_t *grown, *grown_nxt;   // list positions of the cells with more than one candidate that the last pass made, in creation order
    uint16_t *srt, *rk;       // split order -> list position, and list position -> place in the split order (QT_NONE: not to be split)
    int32_t *below;           // counter: places of the split order whose running count is still below the target
    // what the driver reports (the restatement asserts its branches through them)
    int rounds, passes, stop;
};

QT_HD inline int qt_quadrant(const QtCell &c, uint32_t w) {
    const int x = (int)(w & 0xfff), y = (int)((w >> 12) & 0xfff);
    const int mx = c.x0 + ((c.x1 - c.x0 + 1) >> 1), my = c.y0 + ((c.y1 - c.y0 + 1) >> 1);
    return (x < mx ? 0 : 1) + (y < my ? 0 : 2);
}
QT_HD inline QtCell qt_child(const QtCell &c, int q, int n) {
    const int mx = c.x0 + ((c.x1 - c.x0 + 1) >> 1), my = c.y0 + ((c.y1 - c.y0 + 1) >> 1);
    QtCell r;
    r.x0 = (uint16_t)((q & 1) ? mx : c.x0); r.x1 = (uint16_t)((q & 1) ? c.x1 : mx);
    r.y0 = (uint16_t)((q & 2) ? my : c.y0); r.y1 = (uint16_t)((q & 2) ? c.y1 : my);
    r.n = n;
    return r;
}
// non-empty children | children with more than one candidate << 16
QT_HD inline uint32_t qt_nz_gr(const int32_t c[4]) {
    uint32_t v = 0;
    for (int q = 0; q < 4; ++q) v += (c[q] > 0 ? 1u : 0u) + (c[q] > 1 ? 0x10000u : 0u);
    return v;
}

// ---- the bodies -------------------------------------------------------------------------------------------------------------------
// root j of the initial list: box [(int)(h_x j), (int)(h_x (j + 1))) x [0, h), no candidates yet
QT_HD inline void qt_root_cell(QtState &S, const QtSet &set, int j) {
    QtCell c;
    c.x0 = (uint16_t)(int)QT_FMUL(set.h_x, (float)j); c.x1 = (uint16_t)(int)QT_FMUL(set.h_x, (float)(j + 1));
    c.y0 = 0; c.y1 = (uint16_t)set.h; c.n = 0;
    S.cur[j] = c;
}
// candidate i joins root (int)(x / h_x): NOT the root whose box holds x (986 wide, 3 roots: x = 328 is in root 0 = [0, 328))
QT_HD inline void qt_root_cand(QtState &S, const QtSet &set, int i) {
    int r = (int)QT_FDIV((float)(S.word[i] & 0xfff), set.h_x);
    if (r > set.n_ini - 1) r = set.n_ini - 1;
    S.cid[i] = (uint16_t)r;
    QT_ADD(&S.cur[r].n, 1);
}
// before a pass: cell j's quadrant counts, and whether it may split.  full: every cell with more than one candidate, in list order;
// otherwise the cells of `grown` (qt_sort_rank)
QT_HD inline void qt_pass_cell(QtState &S, int j, bool full) {
    for (int q = 0; q < 4; ++q) S.cnt4[j][q] = 0;
    const bool split = full && S.cur[j].n > 1;
    S.rk[j] = split ? (uint16_t)j : QT_NONE;
    if (full) S.srt[j] = (uint16_t)j;
}
// place of grown[e] in the order (size, creation order) descending: the number of entries with a greater key (keys are unique)
QT_HD inline void qt_sort_rank(QtState &S, int e, int g) {
    const int j = S.grown[e], n = S.cur[j].n;
    int r = 0;
    for (int f = 0; f < g; ++f) {
        const int m = S.cur[S.grown[f]].n;
        r += (m > n || (m == n && f > e)) ? 1 : 0;
    }
    S.srt[r] = (uint16_t)j;
    S.rk[j] = (uint16_t)r;
}
QT_HD inline void qt_count_cand(QtState &S, int i) {
    const int c = S.cid[i];
    if (S.rk[c] != QT_NONE) QT_ADD(&S.cnt4[c][qt_quadrant(S.cur[c], S.word[i])], 1);
}
QT_HD inline void qt_scan_input(QtState &S, int r) {
    const int j = S.srt[r];
    S.sc[r] = S.rk[j] == QT_NONE ? 0u : qt_nz_gr(S.cnt4[j]);
}
// (after the exclusive scan of sc) place r's running count: the list's count + non-empty children - 1 of the places up to r
QT_HD inline void qt_below_target(QtState &S, int r, int count, int target) {
    const int j = S.srt[r];
    const int incl = (int)((S.sc[r] + qt_nz_gr(S.cnt4[j])) & 0xffff);
    if (count + incl - (r + 1) < target) QT_ADD(S.below, 1);
}
QT_HD inline void qt_stay_input(QtState &S, int j, int J) { S.sk[j] = S.rk[j] <= J ? 0u : 1u; }     // (QT_NONE > every J)
// write cell j's part of the new list: its children at the front (those of place J first, each cell's in the order SE, SW, NE, NW) and
// into grown_nxt (place 0 first, NW, NE, SW, SE), or itself behind all children; cnt4[j] becomes the new positions
QT_HD inline void qt_write_cell(QtState &S, int j, int J, int total_children) {
    const int r = S.rk[j];
    if (r > J) {
        const int pos = total_children + (int)S.sk[j];
        S.nxt[pos] = S.cur[j];
        S.cnt4[j][0] = pos;
        return;
    }
    const uint32_t own = qt_nz_gr(S.cnt4[j]);
    int at = total_children - (int)((S.sc[r] + own) & 0xffff), g = (int)(S.sc[r] >> 16);
    int pos[4] = {0, 0, 0, 0};
    for (int q = 3; q >= 0; --q)
        if (S.cnt4[j][q] > 0) { pos[q] = at; S.nxt[at++] = qt_child(S.cur[j], q, S.cnt4[j][q]); }
    for (int q = 0; q < 4; ++q)
        if (S.cnt4[j][q] > 1) S.grown_nxt[g++] = (uint16_t)pos[q];
    for (int q = 0; q < 4; ++q) S.cnt4[j][q] = pos[q];
}
QT_HD inline void qt_remap_cand(QtState &S, int i, int J) {
    const int c = S.cid[i];
    S.cid[i] = (uint16_t)S.cnt4[c][S.rk[c] <= J ? qt_quadrant(S.cur[c], S.word[i]) : 0];
}
// the final pick: greatest response of the cell, then the smallest index among those
QT_HD inline void qt_pick_cell(QtState &S, int j) { S.cnt4[j][0] = -1; S.cnt4[j][1] = 0x7fffffff; }
QT_HD inline void qt_pick_max(QtState &S, int i) { QT_MAX(&S.cnt4[S.cid[i]][0], (int32_t)(S.word[i] >> 24)); }
QT_HD inline void qt_pick_min(QtState &S, int i) {
    const int c = S.cid[i];
    if ((int32_t)(S.word[i] >> 24) == S.cnt4[c][0]) QT_MIN(&S.cnt4[c][1], (int32_t)i);
}

// ---- the driver -------------------------------------------------------------------------------------------------------------------
// X runs the steps: X::each(n, f) calls f(i) for every i in [0, n) in any order and completes them all before it returns;
// X::scan(a, n) replaces a[0 .. n) by its exclusive prefix sums and returns the total; X::zero(p) stores 0 to *p.  Every scalar below
// is computed from memory the steps have completed, so on the device every thread of the workgroup holds the same values.
// Returns QT_OK and the list in S.cur[0 .. *count) with cnt4[j][1] = index of cell j's kept candidate, or a status.
template <class X>
QT_HD inline int qt_distribute(X &x, QtState &S, const QtSet &set, int *count_out) {
    S.rounds = S.passes = 0; S.stop = -1;
    *count_out = 0;
    if (S.n <= 0) return QT_OK;
    if (set.n_ini < 1 || set.n_ini > QT_MAX_CELLS) return QT_ERR_CELLS;
    int count = set.n_ini, g = 0;
    x.each(set.n_ini, [&](int j) { qt_root_cell(S, set, j); S.rk[j] = QT_NONE; });
    x.each(S.n, [&](int i) { qt_root_cand(S, set, i); });
    // roots without candidates leave the list: a pass in which no cell splits and the empty ones do not stay
    x.each(count, [&](int j) { S.sk[j] = S.cur[j].n > 0 ? 1u : 0u; });
    {
        const int stay = (int)x.scan(S.sk, count);
        x.each(count, [&](int j) { if (S.cur[j].n > 0) { S.nxt[S.sk[j]] = S.cur[j]; } S.cnt4[j][0] = (int)S.sk[j]; });
        x.each(S.n, [&](int i) { S.cid[i] = (uint16_t)S.cnt4[S.cid[i]][0]; });
        QtCell *t = S.cur; S.cur = S.nxt; S.nxt = t;
        count = stay;
    }
    bool full = true;
    for (int it = 0;; ++it) {
        if (it == QT_MAX_ROUNDS) return QT_ERR_ROUNDS;
        const int before = count, L = full ? count : g;
        if (L == 0) break;                          // nothing left to split: count == before
        if (full) ++S.rounds; else ++S.passes;
        x.zero(S.below);
        x.each(count, [&](int j) { qt_pass_cell(S, j, full); });
        if (!full) x.each(g, [&](int e) { qt_sort_rank(S, e, g); });
        x.each(S.n, [&](int i) { qt_count_cand(S, i); });
        x.each(L, [&](int r) { qt_scan_input(S, r); });
        x.scan(S.sc, L);
        int J = L - 1;
        if (!full) {
            x.each(L, [&](int r) { qt_below_target(S, r, count, set.target); });
            const int b = *S.below;
            J = b < L - 1 ? b : L - 1;
            S.stop = J;
        }
        const uint32_t upto = S.sc[J] + (S.rk[S.srt[J]] == QT_NONE ? 0u : qt_nz_gr(S.cnt4[S.srt[J]]));
        const int total_children = (int)(upto & 0xffff), grown_next = (int)(upto >> 16);
        x.each(count, [&](int j) { qt_stay_input(S, j, J); });
        const int stay = (int)x.scan(S.sk, count);
        if (total_children + stay > QT_MAX_CELLS) return QT_ERR_CELLS;
        x.each(count, [&](int j) { qt_write_cell(S, j, J, total_children); });
        x.each(S.n, [&](int i) { qt_remap_cand(S, i, J); });
        { QtCell *t = S.cur; S.cur = S.nxt; S.nxt = t; }
        { uint16_t *t = S.grown; S.grown = S.grown_nxt; S.grown_nxt = t; }
        count = total_children + stay; g = grown_next;
        if (count >= set.target || count == before) break;
        if (full && count + 3 * g > set.target) full = false;     // close to the target: the most populated cells first
    }
    x.each(count, [&](int j) { qt_pick_cell(S, j); });
    x.each(S.n, [&](int i) { qt_pick_max(S, i); });
    x.each(S.n, [&](int i) { qt_pick_min(S, i); });
    *count_out = count;
    return QT_OK;
}

}  // namespace sivo
