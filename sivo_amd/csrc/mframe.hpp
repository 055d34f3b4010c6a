// mframe.hpp — the device side of a frame (sivo_mframe_t): what search.hip builds and owns, the view of it that a kernel reads
// (MframeView: search.hip's rounds, fuse_batch.hip's table of keyframes), and the device helpers every guided matcher shares: the window
// walk of Frame::GetFeaturesInArea over the frame's grid (scan_window), the (distance, visiting order) key and the Hamming distance.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <vector>

#include "../../include/sivo_hip.h"
#include "grid_math.hpp"

#define SIVO_TH_HIGH 100
#define SIVO_TH_LOW 50

// Device side of a frame: ONE device allocation (keys, descriptors, grid, scale tables, then the engine's scratch), one pinned
// host buffer of the same layout to stage uploads and read results back through, one stream.  Slabs outlive the frames that
// use them: sivo_mframe_destroy hands the slab to a per-process pool and the next sivo_mframe_create on that device takes it
// back, so a tracking loop that builds a frame view per image allocates nothing after its first frames (hipMalloc +
// hipHostMalloc + hipStreamCreate are ~0.3 ms together, more than the searches they would serve).
struct MframeSlab {
    int device = 0;
    char *d = nullptr, *h = nullptr;           // device memory / pinned host mirror
    size_t cap = 0;
    hipStream_t stream = nullptr;
    ~MframeSlab() {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace sivo {
// What a kernel reads of one frame: pointers into its slab, the grid's bounds, the key count.
struct MframeView {
    const float *x, *y, *angle, *ur, *scale, *sigma2, *inv_sigma2;     // ur: null for a frame without mvRight
    const int32_t *oct, *cell_off, *cell_idx;
    const uint4 *desc;
    float min_x, min_y, inv_w, inv_h;
    int32_t n;
};
}  // namespace sivo

struct sivo_mframe {
    int device = 0, n = 0, nlevels = 0;
    float min_x = 0, max_x = 0, min_y = 0, max_y = 0, inv_w = 0, inv_h = 0;
    // host copies (GetFeaturesInArea on the host, wrappers)
    std::vector<SivoKeyPoint> keys;
    std::vector<float> u_right, scale, sigma2, inv_sigma2;
    std::vector<int32_t> cell_off, cell_idx;
    // device (offsets into the slab)
    std::unique_ptr<MframeSlab> slab;
    size_t frame_bytes = 0;                    // the frame's own arrays end here; the engine's scratch follows
    float *d_x = nullptr, *d_y = nullptr, *d_angle = nullptr, *d_ur = nullptr, *d_scale = nullptr, *d_sigma2 = nullptr,
          *d_inv_sigma2 = nullptr;
    int32_t *d_oct = nullptr, *d_cell_off = nullptr, *d_cell_idx = nullptr;
    uint4 *d_desc = nullptr;
    hipStream_t stream = nullptr;
    // The only place that reads the d_* members for a kernel.  A view taken before the engine's scratch() is stale: scratch() can move
    // the frame to a bigger slab, which rebinds every pointer (and the stream).
    sivo::MframeView view() const {
        return sivo::MframeView{d_x, d_y, d_angle, u_right.empty() ? nullptr : d_ur, d_scale, d_sigma2, d_inv_sigma2, d_oct, d_cell_off,
                                d_cell_idx, d_desc, min_x, min_y, inv_w, inv_h, n};
    }
    ~sivo_mframe();
};

namespace sivo {
// Frame::GetFeaturesInArea's walk, the lane's share: visit(idx, order) for every 64th key of the CSR spans the window covers, column by
// column; `order` is the key's position in the reference's walk.  The walk yields every key of the covered CELLS: the in_window test
// (grid_math.hpp) is the visitor's, which may have cheaper rejections to make first.
template <class Visit>
__device__ __forceinline__ void scan_window(const MframeView &V, float u, float v, float r, int lane, Visit visit) {
    int cx0, cx1, cy0, cy1;
    if (!grid_window(V.min_x, V.min_y, V.inv_w, V.inv_h, u, v, r, cx0, cx1, cy0, cy1)) return;
    uint32_t base = 0;
    for (int ix = cx0; ix <= cx1; ++ix) {
        const int s = V.cell_off[ix * SIVO_GRID_ROWS + cy0], e = V.cell_off[ix * SIVO_GRID_ROWS + cy1 + 1];
        for (int j = s + lane; j < e; j += 64) visit(V.cell_idx[j], base + (uint32_t)(j - s));
        base += (uint32_t)(e - s);
    }
}

// The key a wave minimises: distance, then visiting order (< 2^22: the callers' limit on keys and list entries) — the reference's
// first-minimum-wins scan; a caller whose LAST minimum wins passes the order's complement.
constexpr uint32_t KEY_NONE = 0xffffffffu;
__device__ __forceinline__ uint32_t match_key(int d, uint32_t order) { return ((uint32_t)d << 22) | order; }

__device__ __forceinline__ int ham256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
}  // namespace sivo
