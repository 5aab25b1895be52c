// vrc_travel.h -- the travel-distance field of a brick-word field from a set of seeds, and the routes read off it
// (vrc_travel.hip), as vrc_snapshots.hip calls it.  Like the flood and the distance transform it knows arrays only; volumes,
// their ordering and every allocation stay with the entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"

namespace vrc {

// bytes of device scratch a field at `depth` needs: the three 64-bit stats slots, the three tile-flag buffers and the sweep
// counters (vrc.h: vrc_travel_field)
size_t travel_scratch_bytes(uint32_t depth);
// the three stats slots at the start of the scratch: [0] = seeds in M, [1] = voxels with a finite value, [2] = (max_steps << 32)
// | ~dense index of the first voxel that holds it, 0 where no voxel has a finite value
unsigned long long* travel_stats_slots(uint32_t* scratch);
// the hard bound of the sweep loop: max T + 2 <= 8^depth + 1, step_limit + 2 under a limit (the argument: top of vrc_travel.hip)
uint32_t travel_sweep_bound(uint32_t depth, uint32_t step_limit);
// field[(x*S + y)*S + z] = the least number of steps from a seed (a solid voxel of `seeds` that lies in M) to the voxel through
// M (M = the solid voxels of `medium` for through == 0, its empty ones otherwise), VRC_DISTANCE_NONE outside M, where no
// chain exists, and beyond step_limit (0 = none).  Zeroes the scratch, then the init pass, the sweeps and the stats pass.
// Enqueues on `st` and synchronises it: the host decides convergence.  *converged == 0 means the bound was hit.
hipError_t travel_run(const uint32_t* seeds, const uint32_t* medium, uint32_t depth, int connectivity, int through, uint32_t step_limit,
                      uint32_t* field, uint32_t* scratch, hipStream_t st, uint32_t* sweeps, uint32_t* converged);
// lengths[i] = field at start_xyz[3i..3i+2] (VRC_DISTANCE_NONE outside the volume), and where it is finite the route's voxels
// 0 .. min(T, capacity - 1) at paths_xyz[(i*capacity + k)*3 ..]: each next voxel the first neighbour in ascending (dx, dy, dz)
// order whose value is one less
void travel_trace_run(const uint32_t* field, uint32_t depth, int connectivity, uint64_t n, const uint32_t* start_xyz, uint32_t capacity,
                      uint32_t* paths_xyz, uint32_t* lengths, hipStream_t st);

}  // namespace vrc
