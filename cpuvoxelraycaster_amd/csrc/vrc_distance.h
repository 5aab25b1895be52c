// vrc_distance.h -- the exact squared Euclidean distance field of a brick-word field (vrc_distance.hip), as vrc_volume.hip
// calls it.  Like the flood and the labelling it knows arrays only; volumes, their ordering and every allocation stay with
// vrc_volume.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"

namespace vrc {

// bytes of device scratch a transform at `depth` needs on a device of `cu_count` compute units: the two 64-bit stats
// slots, and from 256^3 on the envelope stacks of the lines in flight (vrc.h: vrc_volume_distance_field)
size_t distance_scratch_bytes(uint32_t depth, int cu_count);
// the two stats slots at the start of the scratch: [0] = |F inside the volume|, [1] = (max_d2 << 32) | ~dense index of the
// first voxel that holds it, 0 where no voxel has a finite distance
unsigned long long* distance_stats_slots(uint32_t* scratch);
// field[(x*S + y)*S + z] = the squared distance to the nearest voxel of F (F = the solid voxels of `medium` for to == 0, the
// empty ones otherwise; with outside != 0 every lattice point beyond the faces as well), VRC_DISTANCE_NONE where F is
// empty.  Zeroes the stats slots, then three kernels.  Enqueues on `st`.
void distance_run(const uint32_t* medium, uint32_t depth, int to, int outside, int cu_count, uint32_t* field, uint32_t* scratch, hipStream_t st);
// d2[i] = field at voxel xyz[3i..3i+2], VRC_DISTANCE_NONE outside the volume
void distance_at_run(const uint32_t* field, uint32_t depth, uint64_t n, const uint32_t* xyz, uint32_t* d2, hipStream_t st);
// dst (op)= { p : lo <= field[p] <= hi }, whole words
void distance_select_run(const uint32_t* field, uint32_t depth, uint32_t lo, uint32_t hi, uint32_t* dst, int op, hipStream_t st);

}  // namespace vrc
