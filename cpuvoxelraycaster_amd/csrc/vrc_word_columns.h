// vrc_word_columns.h -- the brick words of the occupancy field read along z: the 40-bit COLUMN form of a brick row that the
// automaton (vrc_cells.hip) and the neighbourhood masks of the voxel lists (vrc_voxels.hip) step through, and the eight
// voxels of one (x, y) out of a word that the distance and travel fields (vrc_distance.hip, vrc_travel.hip) start from.
//
// The layout of a word (2 x 2 x 8 voxels, bit zz*4 + yb*2 + xb) is described at the top of vrc_flood.hip; the masks are
// vrc_flood.h's.  A column is  top nibble of word wz - 1 | word wz | bottom nibble of word wz + 1  in a 64-bit register, so
// that bit 4 + i is bit i of the word and the two z layers beyond it sit below and above: a step along z reads the column
// at bit 0 / 4 / 8, a step along x or y is the flood's shift with the other half from the column of the row that way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vrc_flood.h"

namespace {

constexpr uint64_t X0 = ((uint64_t)vrc::WORD_X0 << 32) | vrc::WORD_X0, X1 = ~X0;
constexpr uint64_t Y0 = ((uint64_t)vrc::WORD_Y0 << 32) | vrc::WORD_Y0, Y1 = ~Y0;

// the field the columns are read from: 2^lg brick rows per axis, edge = all ones where beyond the volume is solid
struct WordColumns {
    const uint32_t* __restrict__ words;
    uint32_t lg, edge;
};

// The column of brick row (cx, cy) at word wz; rows and nibbles beyond the volume's faces are all `edge`.  SMALL (4^3,
// lg = 1): the half cy of word cx between two nibbles of `edge`, 24 bits.  WITH_Z = false leaves the z-neighbour words
// alone, for the rows of which only the word itself is used.
template <bool SMALL, bool WITH_Z>
__device__ __forceinline__ uint64_t column(const WordColumns& f, int32_t cx, int32_t cy, uint32_t wz)
{
    const uint64_t edge4 = f.edge & 0xFu;
    const int32_t n = 1 << f.lg;
    if (cx < 0 || cy < 0 || cx >= n || cy >= n) return f.edge ? ~0ull : 0ull;
    if (SMALL) {
        const uint64_t half = (f.words[cx] >> (16u * (uint32_t)cy)) & 0xffffu;
        return edge4 | (half << 4) | (edge4 << 20);
    }
    const uint32_t lgz = f.lg - 2u;
    const uint32_t* row = f.words + ((((uint32_t)cx << f.lg) + (uint32_t)cy) << lgz);     // below 2^25
    uint64_t below = edge4, above = edge4;
    if (WITH_Z) {
        if (wz > 0u) below = row[wz - 1u] >> 28;
        if (wz + 1u < (1u << lgz)) above = row[wz + 1u] & 0xFu;
    }
    return below | ((uint64_t)row[wz] << 4) | (above << 36);
}

// the voxel one step before / after along x or y, at this voxel's bit position: c = this row, o = the row that way
__device__ __forceinline__ uint64_t x_before(uint64_t c, uint64_t o) { return ((c & X0) << 1) | ((o & X1) >> 1); }
__device__ __forceinline__ uint64_t x_after(uint64_t c, uint64_t o) { return ((c & X1) >> 1) | ((o & X0) << 1); }
__device__ __forceinline__ uint64_t y_before(uint64_t c, uint64_t o) { return ((c & Y0) << 2) | ((o & Y1) >> 2); }
__device__ __forceinline__ uint64_t y_after(uint64_t c, uint64_t o) { return ((c & Y1) >> 2) | ((o & Y0) << 2); }

// the 8 voxels (x&1, y&1 = sh) of the 4 brick bytes of a word, z ascending
__device__ __forceinline__ uint32_t column_bits_of_word(uint32_t w, uint32_t sh)
{
    uint32_t t = (w >> sh) & 0x11111111u;     // bit 0 / 4 of every byte: z even / odd
    t = (t | (t >> 3)) & 0x03030303u;
    t = (t | (t >> 6)) & 0x000f000fu;
    return (t | (t >> 12)) & 0xffu;
}

}  // namespace
