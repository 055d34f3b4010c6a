// mframe.hpp — the device side of a frame (sivo_mframe_t): what search.hip builds and owns, and what fuse_batch.hip reads of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <vector>

#include "../../include/sivo_hip.h"

#define SIVO_GRID_COLS 64   // FRAME_GRID_COLS (reference include/orbslam/Frame.h:38-39)
#define SIVO_GRID_ROWS 48
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
    ~sivo_mframe();
};

namespace sivo {
__device__ __forceinline__ int ham256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
}  // namespace sivo
