// vrc_box_words.h -- the brick-byte field's addressing, and a clipped voxel box as a list of the 32-bit occupancy words its
// brick rows touch: the work layout of every kernel that edits or reads a box of the field (vrc_volume.hip: boxes, spheres,
// region copy, box counts; vrc_stamp.hip: the affine stamp), the launch that goes with it, and the two ways a kernel writes
// a destination word under VRC_COPY_REPLACE / OR / ANDNOT.  A word holds four bricks along z, 2 x 2 x 8 voxels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"

namespace {

// the byte index of the brick that holds voxel (x, y, z) in a field of n bricks per axis, and the voxel's bit in that byte
__host__ __device__ __forceinline__ uint64_t brick_of(uint32_t n, uint32_t x, uint32_t y, uint32_t z)
{
    return ((uint64_t)(x >> 1) * n + (y >> 1)) * n + (z >> 1);
}
__host__ __device__ __forceinline__ uint32_t voxel_bit(uint32_t x, uint32_t y, uint32_t z) { return (z & 1u) * 4u + (y & 1u) * 2u + (x & 1u); }

// A voxel's KEY is its bit index in the field, 8 B + (z&1) 4 + (y&1) 2 + (x&1) with B its brick's byte index: the index of the
// per-voxel arrays (the labels).  lg = log2 of the bricks per axis.
__host__ __device__ __forceinline__ uint32_t voxel_key(uint32_t lg, uint32_t x, uint32_t y, uint32_t z)
{
    return 8u * ((((x >> 1) << lg | (y >> 1)) << lg) | (z >> 1)) + voxel_bit(x, y, z);
}
__host__ __device__ __forceinline__ void key_voxel(uint32_t lg, uint32_t key, uint32_t c[3])
{
    const uint32_t B = key >> 3, nm = (1u << lg) - 1u;
    c[0] = 2u * (B >> (2u * lg)) + (key & 1u);
    c[1] = 2u * ((B >> lg) & nm) + ((key >> 1) & 1u);
    c[2] = 2u * (B & nm) + ((key >> 2) & 1u);
}

// lo_hi[0..5] clipped to the volume; false = empty, inverted or wholly outside
__host__ __device__ __forceinline__ bool clip_box(const uint32_t* lo_hi, uint32_t S, uint32_t lo[3], uint32_t hi[3])
{
    for (int a = 0; a < 3; ++a) {
        lo[a] = lo_hi[a];
        hi[a] = lo_hi[3 + a] < S ? lo_hi[3 + a] : S;
        if (lo[a] >= hi[a]) return false;
    }
    return true;
}

// the voxels of brick coordinate c (one axis) that lie in [lo, hi): bit 0 = voxel 2c, bit 1 = voxel 2c + 1
__device__ __forceinline__ uint32_t axis_pair(uint32_t c, uint32_t lo, uint32_t hi)
{
    const uint32_t v = 2u * c;
    return ((v >= lo && v < hi) ? 1u : 0u) | ((v + 1u >= lo && v + 1u < hi) ? 2u : 0u);
}

// The brick rows a clipped, non-empty voxel box [lo, hi) touches, as a list of work items.  A row = the bricks
// (cx, cy, cz0..cz1), contiguous bytes; item = (row, k-th 32-bit word of the row).
struct BoxWords {
    uint32_t lo[3], hi[3];
    uint32_t bx0, by0, cz0, cz1, nby, wpr;
    uint64_t items;
};

// The number of work items of a clipped, non-empty box: for the host to size a launch by, and for box_words below, so that
// the two agree by construction.
__host__ __device__ __forceinline__ uint64_t box_word_items(const uint32_t lo[3], const uint32_t hi[3])
{
    const uint32_t nbx = ((hi[0] - 1u) >> 1) - (lo[0] >> 1) + 1u, nby = ((hi[1] - 1u) >> 1) - (lo[1] >> 1) + 1u;
    const uint32_t wpr = (((((hi[2] - 1u) >> 1) - (lo[2] >> 1)) + 3u) >> 2) + 1u;
    return (uint64_t)nbx * nby * wpr;
}

// the launch of the kernels that take ONE box: a thread per word of the box's rows, at most 16384 groups of 256, the rest by
// grid stride
inline uint32_t box_launch_groups(const uint32_t lo[3], const uint32_t hi[3])
{
    const uint64_t groups = (box_word_items(lo, hi) + 255u) / 256u;
    return groups > 16384u ? 16384u : (uint32_t)groups;
}

__device__ __forceinline__ BoxWords box_words(const uint32_t lo[3], const uint32_t hi[3])
{
    BoxWords b;
    for (int a = 0; a < 3; ++a) { b.lo[a] = lo[a]; b.hi[a] = hi[a]; }
    b.bx0 = lo[0] >> 1; b.by0 = lo[1] >> 1; b.cz0 = lo[2] >> 1;
    b.nby = ((hi[1] - 1u) >> 1) - b.by0 + 1u;
    b.cz1 = (hi[2] - 1u) >> 1;
    b.wpr = ((b.cz1 - b.cz0 + 3u) >> 2) + 1u;          // upper bound of the words one row touches, whatever its alignment
    b.items = box_word_items(lo, hi);
    return b;
}

// One item of a box: the word index `w`, the row's brick coordinates and the byte indices of brick (cx, cy, 0) and of
// the row's first / last brick.  false: the row has fewer words than wpr and this item is beyond them.
struct RowWord {
    uint32_t cx, cy;
    uint64_t base, first, last, w;
};

__device__ __forceinline__ bool row_word(const BoxWords& b, uint32_t n, uint64_t it, RowWord& r)
{
    const uint32_t k = (uint32_t)(it % b.wpr);
    const uint32_t row = (uint32_t)(it / b.wpr);
    r.cx = b.bx0 + row / b.nby; r.cy = b.by0 + row % b.nby;
    r.base = ((uint64_t)r.cx * n + r.cy) * n;
    r.first = r.base + b.cz0; r.last = r.base + b.cz1;
    r.w = (r.first >> 2) + k;
    return r.w <= (r.last >> 2);
}

// the voxels of word r.w that lie inside the box, as a mask of the word's bits
__device__ __forceinline__ uint32_t box_mask(const BoxWords& b, const RowWord& r)
{
    const uint32_t xy = axis_pair(r.cx, b.lo[0], b.hi[0]) | (axis_pair(r.cy, b.lo[1], b.hi[1]) << 2);
    // xy: bit 0 / 1 = x voxel 0 / 1 inside, bit 2 / 3 = y voxel 0 / 1 inside -> the 4 (y, x) bits of one z layer
    const uint32_t layer = ((xy & 1u) ? 0x5u : 0u) | ((xy & 2u) ? 0xAu : 0u);
    const uint32_t plane = (layer & ((xy & 4u) ? 0x3u : 0u)) | (layer & ((xy & 8u) ? 0xCu : 0u));
    uint32_t mask = 0u;
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint64_t byte = 4u * r.w + j;
        if (byte < r.first || byte > r.last) continue;
        const uint32_t zp = axis_pair((uint32_t)(byte - r.base), b.lo[2], b.hi[2]);
        const uint32_t m8 = ((zp & 1u) ? plane : 0u) | ((zp & 2u) ? plane << 4 : 0u);
        mask |= m8 << (8u * j);
    }
    return mask;
}

// dst[w] takes (op) `bits` under `mask` (bits & ~mask == 0): the end of the kernels that gather a box's destination words.
// A word has one owner within a call and is written once, a partly covered one as a masked read-modify-write -- unless
// `shared`: in a volume of 4^3 (n < 4) two brick rows share a word, and its rows take 32-bit vector atomics.
__device__ __forceinline__ void store_box_word(uint32_t* __restrict__ dst, uint64_t w, uint32_t mask, uint32_t bits, int op, bool shared)
{
    if (shared) {
        if (op == VRC_COPY_REPLACE) { atomicAnd(&dst[w], ~mask); atomicOr(&dst[w], bits); }
        else if (op == VRC_COPY_OR) atomicOr(&dst[w], bits);
        else atomicAnd(&dst[w], ~bits);
        return;
    }
    uint32_t v;
    if (op == VRC_COPY_REPLACE) v = mask == 0xffffffffu ? bits : ((dst[w] & ~mask) | bits);
    else if (op == VRC_COPY_OR) { if (!bits) return; v = dst[w] | bits; }
    else { if (!bits) return; v = dst[w] & ~bits; }
    dst[w] = v;
}

// dst[w] takes (op) the selection K of all 32 voxels of the word: the end of the kernels that select a whole field.  The
// word has a single owner and is written whole with a plain store.
__device__ __forceinline__ void store_selected_word(uint32_t* __restrict__ dst, uint32_t w, uint32_t K, int op)
{
    if (op == VRC_COPY_REPLACE) dst[w] = K;
    else if (!K) return;
    else if (op == VRC_COPY_OR) dst[w] |= K;
    else dst[w] &= ~K;
}

}  // namespace
