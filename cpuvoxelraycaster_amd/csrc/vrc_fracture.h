// vrc_fracture.h -- the Voronoi cell of every voxel around a list of sites (vrc_fracture.hip), as vrc_snapshots.hip calls it
// for vrc_fracture_label.  Like the distance transform and the labelling it knows plain arrays only; volumes, their ordering
// and every allocation stay with the caller.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"

namespace vrc {

// bytes of device scratch the cells of `n_sites` sites at `depth` need on a device of `cu_count` compute units, beside the
// dense cell field itself: the site table (4 bytes per site, rounded up to 16) and, from 256^3 on, the envelope stacks of the
// lines in flight (vrc.h: vrc_fracture_label)
size_t fracture_scratch_bytes(uint32_t depth, int cu_count, uint64_t n_sites);
// cells[(x*S + y)*S + z] = the index of the in-volume site nearest to the voxel, the lowest index among several nearest;
// VRC_NO_COMPONENT where no site lies in the volume or the least squared distance exceeds max_d2 (VRC_DISTANCE_NONE: no
// cut-off).  sites: n_sites x 3 int32 in device memory.  A fill, the scatter and three passes.  Enqueues on `st`.
void fracture_cells_run(const int32_t* sites, uint64_t n_sites, uint32_t depth, uint32_t max_d2, int cu_count, uint32_t* cells, uint32_t* scratch,
                        hipStream_t st);
// piece_cells[id] = cells at records[id].first
void fracture_piece_cells_run(const vrc_component* records, uint64_t count, const uint32_t* cells, uint32_t depth, uint32_t* piece_cells, hipStream_t st);

}  // namespace vrc
