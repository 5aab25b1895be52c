// vrc_cells.h -- one step of a neighbour-count automaton over a brick-word field and the seeded random fill of a box
// (vrc_cells.hip), as vrc_volume_ops.hip calls them.  The kernels know word arrays only; volumes and their ordering stay
// with vrc_volume_ops.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vrc {

// dst = the rule of include/vrc.h (vrc_cells_step) applied to src, two fields of `depth` that do not overlap; every word
// of dst is written once.  neighbours = 6 or 26, outside = 0 or 1, no mask bit above bit `neighbours`.  changed: nullptr,
// or a device counter that the launch ADDS the number of voxels with dst != src to (the caller zeroes it on `st` first).
// One kernel on `st`.
void cells_step_run(uint32_t* dst, const uint32_t* src, uint32_t depth, int neighbours, uint32_t birth_mask, uint32_t survive_mask,
                    int outside, unsigned long long* changed, hipStream_t st);
// The voxels of the clipped, non-empty box [lo, hi) of the field `words` take (op) R(p) = (h(x, y, z) < threshold),
// threshold <= 2^32 (the hash: include/vrc.h, vrc_cells_fill_random).  One kernel on `st`.
void cells_fill_random_run(uint32_t* words, uint32_t depth, uint32_t seed, uint64_t threshold, const uint32_t lo[3], const uint32_t hi[3],
                           int op, hipStream_t st);

}  // namespace vrc
