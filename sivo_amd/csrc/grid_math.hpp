// grid_math.hpp — the frame grid of the reference (src/orbslam/Frame.cc:205-221 AssignFeaturesToGrid, :392-404 PosInGrid, :326-390
// GetFeaturesInArea) and the chi-square gate of ORBmatcher::Fuse (ORBmatcher.cc:878-899), stated once: shared by the kernels
// (search.hip, fuse_batch.hip through mframe.hpp), by the library's host side and, compiled by g++, by the host programs of the tests.
// The grid is a CSR laid out column-major like the reference's mGrid[ix][iy] walk: the cells of one grid column that a window covers
// are one contiguous span of cell_idx.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/sivo_hip.h"

#ifndef SIVO_HD
#ifdef __HIPCC__
#define SIVO_HD __host__ __device__ inline
#else
#define SIVO_HD inline
#endif
#endif

#define SIVO_GRID_COLS 64   // FRAME_GRID_COLS (reference include/orbslam/Frame.h:38-39)
#define SIVO_GRID_ROWS 48

namespace sivo {

// Frame.cc:334-357: the cell range [cx0, cx1] x [cy0, cy1] of the window (u, v, r); false when the window misses the grid.
SIVO_HD bool grid_window(float min_x, float min_y, float inv_w, float inv_h, float u, float v, float r, int &cx0, int &cx1, int &cy0,
                         int &cy1) {
    const int x0 = (int)floorf((u - min_x - r) * inv_w), x1 = (int)ceilf((u - min_x + r) * inv_w);
    const int y0 = (int)floorf((v - min_y - r) * inv_h), y1 = (int)ceilf((v - min_y + r) * inv_h);
    cx0 = x0 > 0 ? x0 : 0;
    cx1 = x1 < SIVO_GRID_COLS - 1 ? x1 : SIVO_GRID_COLS - 1;
    cy0 = y0 > 0 ? y0 : 0;
    cy1 = y1 < SIVO_GRID_ROWS - 1 ? y1 : SIVO_GRID_ROWS - 1;
    return cx0 < SIVO_GRID_COLS && cx1 >= 0 && cy0 < SIVO_GRID_ROWS && cy1 >= 0;
}

// Frame.cc:379-384: the key (kx, ky) of a covered cell lies inside the window
SIVO_HD bool in_window(float kx, float ky, float u, float v, float r) {
    return fabsf(kx - u) < r && fabsf(ky - v) < r;
}

// ORBmatcher.cc:878-899: whether the candidate passes.  (ex, ey) = projection - key, er = projected ur - the key's (read only with
// has_right: the key has a right coordinate); the error is summed and scaled in float and compared in double, as the reference does.
// (Two branches with a return each, as the reference's two `continue`s: folded into one select the kernels need 3-4 more VGPRs, which
// costs fuse_batch_kernel a wave per SIMD.)
SIVO_HD bool fuse_chi2_gate(float ex, float ey, bool has_right, float er, float inv_sigma2) {
    if (has_right) {
        const float e2 = ex * ex + ey * ey + er * er;
        if ((double)(e2 * inv_sigma2) > 7.8) return false;
    } else {
        const float e2 = ex * ex + ey * ey;
        if ((double)(e2 * inv_sigma2) > 5.99) return false;
    }
    return true;
}

// AssignFeaturesToGrid + PosInGrid -> CSR in mGrid[ix][iy] order (host only).  A key whose rounded cell lies outside the grid is in no
// cell; within a cell the keys stand in index order, as the reference's push_back leaves them.
inline void grid_build(const SivoKeyPoint *keys, int n, float min_x, float min_y, float inv_w, float inv_h, std::vector<int32_t> &cell_off,
                       std::vector<int32_t> &cell_idx) {
    const int cells = SIVO_GRID_COLS * SIVO_GRID_ROWS;
    std::vector<int32_t> cell_of((size_t)n, -1);
    cell_off.assign((size_t)cells + 1, 0);
    for (int i = 0; i < n; ++i) {
        const int px = (int)roundf((keys[i].x - min_x) * inv_w), py = (int)roundf((keys[i].y - min_y) * inv_h);
        if (px < 0 || px >= SIVO_GRID_COLS || py < 0 || py >= SIVO_GRID_ROWS) continue;
        cell_of[(size_t)i] = px * SIVO_GRID_ROWS + py;
        ++cell_off[(size_t)cell_of[(size_t)i] + 1];
    }
    for (int c = 0; c < cells; ++c) cell_off[(size_t)c + 1] += cell_off[(size_t)c];
    cell_idx.assign((size_t)cell_off[(size_t)cells], 0);
    std::vector<int32_t> fill(cell_off.begin(), cell_off.end() - 1);
    for (int i = 0; i < n; ++i)
        if (cell_of[(size_t)i] >= 0) cell_idx[(size_t)fill[(size_t)cell_of[(size_t)i]]++] = i;
}

}  // namespace sivo
