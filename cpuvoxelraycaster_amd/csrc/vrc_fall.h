// vrc_fall.h -- how far the pieces of a labelling can fall as rigid bodies, and the scatter that writes every piece moved by
// its own offset (vrc_fall.hip), as vrc_snapshots.hip calls them.  Like the flood and the travel field it knows arrays only;
// volumes, their ordering and every allocation stay with the entry points.  The first part needs no device: the step of a
// face code and the bound of the round loop, for the entry points and for host code that wants them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"

namespace vrc {

// an offset component beyond this in either direction drops the piece whole (vrc.h: vrc_fall_place)
constexpr int32_t PLACE_OFFSET_LIMIT = 1 << 20;

// direction = 2 * axis + side: the unit step g is -e_axis for side 0 and +e_axis for side 1
inline uint32_t fall_axis(int direction) { return (uint32_t)direction >> 1; }
inline int32_t fall_sign(int direction) { return (direction & 1) ? 1 : -1; }
// The hard bound of the round loop.  A round lowers every D[i] to the least bound its constraints give from the values of
// the round before (or newer ones), so after round r every piece whose tightest chain of constraints has at most r links
// (the wall, F or the limit counting as the first) is final; a chain without a repeated piece has at most C links, so round
// C leaves every value final and round C + 1 changes nothing.
inline uint64_t fall_round_bound(uint64_t pieces) { return pieces + 1u; }

// bytes of device scratch a fall over C pieces needs: one uint32 per piece, the changed flag, the union of the pieces'
// boxes and the stats
size_t fall_scratch_bytes(uint64_t pieces);
// offsets[3i .. 3i+2] = D_i * g for the C pieces of `labels` (8^depth ids by key, `records` their C records), F = the solid
// voxels of the word field `fixed` (nullptr: empty), D the greatest drops of vrc.h: vrc_fall_drops.  offsets is DEVICE
// memory.  Enqueues on `st` and synchronises it: the host decides convergence.  *converged == 0 means the bound was hit and
// offsets was not written.  C >= 1.
hipError_t fall_run(const uint32_t* labels, const vrc_component* records, uint64_t pieces, uint32_t depth, const uint32_t* fixed,
                    int direction, uint32_t drop_limit, int32_t* offsets, uint32_t* scratch, hipStream_t st, vrc_fall_stats* stats,
                    uint32_t* converged);
// every voxel p of the labels' set with keep[id(p)] != 0 (keep == nullptr: all) sets (VRC_COPY_OR) or clears
// (VRC_COPY_ANDNOT) voxel p + offsets[id(p)] of the word field dst; targets outside the volume are dropped.  Enqueues on `st`.
void place_run(const uint32_t* labels, uint32_t depth, const uint8_t* keep, const int32_t* offsets, uint32_t* dst, int op, hipStream_t st);

}  // namespace vrc
