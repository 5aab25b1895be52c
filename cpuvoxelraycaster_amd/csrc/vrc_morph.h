// vrc_morph.h -- dilation and erosion of a brick-word field by a structuring element given as a list of offsets
// (vrc_morph.hip), as vrc_volume_ops.hip calls them.  The kernels know word arrays only; volumes, their ordering and the
// block's owner stay with vrc_volume_ops.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vrc {

// The prepared element, one block of MORPH_BLOCK_BYTES in device memory that every call writes anew:
//   33 x 33 columns (ex + 16, ey + 16), one 64-bit z mask each with bit ez + 16          8712 bytes
//   8 words: the number of non-empty columns, the element's box x0 x1 y0 y1 z0 z1, 0     32 bytes
//   the non-empty columns, (ex + 16) | (ey + 16) << 8 each, in no particular order       at most 4356 bytes
constexpr uint32_t MORPH_SIDE = 33u, MORPH_COLUMNS = MORPH_SIDE * MORPH_SIDE;
constexpr size_t MORPH_BLOCK_BYTES = 13312u;

// dst (op)= K of the rule of include/vrc.h (vrc_morph_apply), two fields of `depth` that do not overlap; every word of dst
// is stored once.  d_offsets: n x 3 int32 in device memory (nullptr with n == 0), n <= 2^20; origin: 3 host ints;
// erode, of_empty, outside: 0 or 1.  A memset and three kernels on `st` (two with n == 0).
hipError_t morph_run(uint32_t* dst, const uint32_t* src, uint32_t depth, int erode, int of_empty, int outside, uint64_t n, const int32_t* d_offsets,
                     const int32_t origin[3], int op, void* d_block, hipStream_t st);

}  // namespace vrc
