// vrc_stamp.h -- the affine stamp of one brick-word field into another (vrc_stamp.hip), as vrc_volume.hip calls it.  Like
// the flood and the distance field it knows arrays only; volumes, their ordering and the argument checks stay with
// vrc_volume.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"

namespace vrc {

// dst voxel p of the box [lo, hi) -- clipped to dst and not empty -- takes (op) the src voxel (m (2p + 1) + t) >> 17, 0
// where that lies outside src (vrc.h: vrc_volume_stamp_affine; |m| <= 2^20 and |t| <= 2^40 checked by the caller).  One
// kernel, no scratch.  Enqueues on `st`.
void stamp_affine_run(uint32_t* dst, uint32_t dst_depth, const uint32_t* src, uint32_t src_depth, const vrc_affine& map, const uint32_t lo[3],
                      const uint32_t hi[3], int op, hipStream_t st);

}  // namespace vrc
