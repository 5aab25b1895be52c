// vrc_levels.h -- the counts of the 2^k cubes of a brick-word field, the field of a smaller depth selected by those counts
// and the field of a greater depth that repeats every voxel (vrc_levels.hip), as vrc_volume_ops.hip calls them.  The kernels
// know word arrays only; volumes and their ordering stay with vrc_volume_ops.hip.
//
// A CELL of level k is the cube of 2^k voxels per axis at a multiple of 2^k, 8^k / 8 brick bytes: c = 2^(k-1) bricks per axis,
// c x c brick rows of c contiguous bytes.  Which kernel counts a cell goes by its size, and the switches are where the next
// larger unit of work begins to fit a cell:
//   k = 1       a cell is one byte.  counts: a lane per source word, four counts in one 16-byte store.  reduce: a lane per
//               destination word, which is four rows of eight contiguous source bytes, and a 9-bit table of the band.
//   k = 2, 3    a cell is 2 x 2 rows of two bytes, or 4 x 4 rows of one aligned word: a lane per cell sums the popcounts in
//               registers, adjacent lanes along z take adjacent bytes.
//   k >= 4      a cell is 128 words and more: LEVELS_GROUP_WORDS = 2048 words of a cell to a workgroup (eight per lane),
//               summed over the group (vrc_group.h).  Up to k = 5 (1024 words) that is the whole cell and the count is stored;
//               from k = 6 (8192 words) a cell has several workgroups, whose sums meet in a 32-bit vector atomicAdd on counts
//               zeroed on the stream before -- a sum of integers, so the bytes do not depend on the order.
// reduce for k = 2, 3 counts the cell of every destination voxel in its own lane; for k >= 4 it runs the counts into a scratch
// array of the caller's (levels_scratch_bytes: at most 64^3 counts, the destination has depth 6 at the most) and compares them
// in a second kernel.  Either way a lane owns one destination VOXEL, the 32 lanes of a half-wave are the bits of one word in
// bit order, and the word is one ballot, stored whole by the half-wave's first lane.  4^3 keeps two brick rows in a word; there
// a lane's bit names the row too, so that word has one owner as well and nothing takes atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vrc {

constexpr uint32_t LEVELS_GROUP_WORDS = 2048;     // words of a cell that one workgroup of 256 lanes sums

// counts[(X * Sc + Y) * Sc + Z] = the solid voxels of cell (X, Y, Z) of level k of the field `src` of `depth`, Sc = 2^(depth - k),
// 1 <= k <= depth.  A memset (k >= 6 only) and one kernel on `st`; returns what the memset returned.
hipError_t levels_counts_run(const uint32_t* src, uint32_t depth, uint32_t k, uint32_t* counts, hipStream_t st);

// the bytes of `scratch` that levels_reduce_run asks for: 0 below k = 4
size_t levels_scratch_bytes(uint32_t src_depth, uint32_t k);
// The field dst of depth src_depth - k takes (op) K = { P : lo <= count(P) < hi }, count as above; lo and hi at most 8^k + 1,
// every word of dst has one owner.  k < 4: one kernel; else levels_counts_run into `scratch` and one kernel.
hipError_t levels_reduce_run(uint32_t* dst, const uint32_t* src, uint32_t src_depth, uint32_t k, uint32_t lo, uint32_t hi, int op, uint32_t* scratch,
                             hipStream_t st);

// The field dst of dst_depth takes (op) E = { p : src(p >> k) solid }, src of depth dst_depth - k >= 2, k >= 1.  One kernel.
void levels_expand_run(uint32_t* dst, uint32_t dst_depth, const uint32_t* src, uint32_t k, int op, hipStream_t st);

}  // namespace vrc
