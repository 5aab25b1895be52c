// vrc_sight.h -- straight-line walks over a distance or travel field (vrc_sight.hip), as vrc_snapshots.hip calls them.  Like
// the distance transform it knows arrays only; snapshots, their ordering and every allocation stay with the entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"

namespace vrc {

// the least c with c * c >= lo: what the stride takes off a voxel's free radius (the stride bound)
uint32_t sight_root_above(uint32_t lo);
// out[i] = the record of the walk segments[6i..6i+2] -> segments[6i+3..6i+5] over `field` with the clear band [lo, hi] (the
// rule: include/vrc.h).  touch: the supercover.  stride: the walk may jump where the field's own values prove every voxel it
// passes clear -- the caller gives it only for a field made by vrc_volume_distance_field, the squared distance to a set, with
// hi == 0xffffffff; the records are the plain walk's.
void sight_segments_run(const uint32_t* field, uint32_t depth, uint64_t n, const int32_t* segments, uint32_t lo, uint32_t hi, bool touch, bool stride,
                        vrc_sight* out, hipStream_t st);
// out[(x*S + y)*S + z] = |p - eye|^2 where p is in range (radius == 0: everywhere) and every voxel of the walk eye -> p but p
// itself is clear, VRC_DISTANCE_NONE elsewhere, 0 at the eye.  stats[0] += the finite values, stats[1] = max (value << 32) |
// ~dense index over them; the caller zeroes both.  One lane per voxel, walking towards the eye.
void sight_field_run(const uint32_t* field, uint32_t depth, const uint32_t eye[3], uint32_t radius, uint32_t lo, uint32_t hi, bool touch, bool stride,
                     uint32_t* out, unsigned long long* stats, hipStream_t st);

}  // namespace vrc
