// vrc_voxelize.h -- solid voxelisation of triangle meshes into a brick-word field (vrc_voxelize.hip), as vrc_volume.hip
// calls it.  The voxeliser knows word arrays only; volumes, their ordering, staging and scratch memory stay with
// vrc_volume.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vrc {

// bytes of the mark field a voxelisation at `depth` needs: the occupancy's own layout and size
size_t voxelize_scratch_bytes(uint32_t depth);
// occupancy ^= the crossing parity of the n triangles (n x 9 int32 in device memory, include/vrc.h: vrc_volume_xor_mesh).
// `marks` is all zero on entry and all zero again when the second kernel has run.  Enqueues two kernels on `st`; n >= 1.
void voxelize_run(uint32_t* occupancy, uint32_t* marks, uint32_t depth, uint64_t n, const int32_t* tris, hipStream_t st);

}  // namespace vrc
