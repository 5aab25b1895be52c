// vrc_flood.h -- flood fill by connectivity over two brick-word fields (vrc_flood.hip), as vrc_volume.hip calls it.
// The flood knows word arrays only; volumes, their ordering and their scratch memory stay with vrc_volume.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vrc {

// The voxels of a word with x = 0 / x = 1 and with y = 0 / y = 1 inside their brick (the layout: top of vrc_flood.hip): a
// one-voxel step along x is a shift by 1 under WORD_X0 / WORD_X1, along y by 2 under WORD_Y0 / WORD_Y1, along z by 4.
constexpr uint32_t WORD_X0 = 0x55555555u, WORD_X1 = 0xAAAAAAAAu, WORD_Y0 = 0x33333333u, WORD_Y1 = 0xCCCCCCCCu;

// bytes of device scratch a flood at `depth` needs (tile flags and sweep counters)
size_t flood_scratch_bytes(uint32_t depth);
// the library's own sweep bound for max_sweeps == 0 (include/vrc.h: vrc_volume_flood)
uint32_t flood_sweep_bound(uint32_t depth);
// region |= everything of M joined to region & M, M = medium (through == 0) or its complement inside the volume.
// Enqueues on `st` and synchronises it: the host decides convergence.  max_sweeps >= 1.
hipError_t flood_run(uint32_t* region, const uint32_t* medium, uint32_t depth, int connectivity, int through, uint32_t max_sweeps,
                     uint32_t* scratch, hipStream_t st, uint32_t* sweeps, uint32_t* converged);

}  // namespace vrc
