// orb_quadtree.hpp — the device quadtree's launcher, shared between orb_quadtree.hip (kernel, sivo_orb_distribute_batch_dev) and
// orb.hip (launch-mode bit 4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orb_quadtree_math.hpp"

namespace sivo {

// One workgroup per set.  `off` is the offset table the sets' off_b / off_e index, `words` the packed candidates it delimits (either
// may be host memory the device can address); an offset outside [0, off_limit] gives that set QT_ERR_OFFSETS.  work_words / work_ids:
// device scratch for off_limit candidates.  Per set s: the kept words in list order at out_words[slot_base ..], their indices inside
// the set at out_idx[slot_base ..] (may be NULL), the count at out_count[s], QT_OK or the reason there is no list at out_status[s].
void quadtree_launch(hipStream_t st, int n_sets, const QtSet *d_sets, const int32_t *off, int32_t off_limit, const uint32_t *words,
                     uint32_t *work_words, uint16_t *work_ids, uint32_t *out_words, int32_t *out_idx, int32_t *out_count,
                     int32_t *out_status);

// n_ini = round(w / h) (halves away from zero) and h_x = (float)w / n_ini, as ORBextractor.cc:546-549 computes them
void quadtree_roots(int w, int h, int *n_ini, float *h_x);

const char *quadtree_status_text(int status);

}  // namespace sivo
