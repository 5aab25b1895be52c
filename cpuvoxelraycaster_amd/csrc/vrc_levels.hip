// vrc_levels.hip -- voxels between volumes of two depths (include/vrc.h: vrc_levels_counts, vrc_levels_reduce,
// vrc_levels_expand): the number of solid voxels in every 2^k cube, the coarse volume those counts select, and the fine
// volume that repeats every coarse voxel 2^k times per axis.
//
// The layout: a brick byte is 2 x 2 x 2 voxels, bit zb*4 + yb*2 + xb, at [(cx*n + cy)*n + cz]; a word is four bricks along z,
// 2 x 2 x 8 voxels with bit 4 zz + 2 yb + xb (the top of vrc_flood.hip).  A cell of level k is c = 2^(k-1) bricks per axis, so
// its count is the sum of the popcounts of c x c pieces of brick rows, c bytes each; counts are dense, [(X*Sc + Y)*Sc + Z],
// which for k = 1 is the order of the brick bytes themselves.  Which kernel takes which k, and why: vrc_levels.h.
//
// Reduce.  Voxel (X, Y, Z) of dst is cell (X, Y, Z) of src.  For k = 1 the 32 voxels of dst word (cx, cy, wz) are the source
// bytes 8 wz .. 8 wz + 7 of the four rows (2 cx + xb, 2 cy + yb): a lane per word loads them as four 8-byte values and looks
// every popcount up in a 9-bit table of the band.  Otherwise a lane per dst voxel, numbered so that lane i holds bit i & 31 of
// word i >> 5: the word is the half-wave's share of one ballot.  In 4^3 (two words) bit 16 cy + 4 z + 2 yb + xb holds the row cy.
// Expand.  A lane per dst word.  Every dst brick is uniform for k >= 1: brick (cx, cy, cz) is 0xff or 0x00 with the source
// voxel (cx, cy, cz) >> (k - 1), so the lane reads one byte per distinct source brick along z, at most four.
// Every launch is 256-lane groups, at most 16384 of them, the rest by grid stride; no kernel stores a word it does not own.
#include "vrc_levels.h"

#include "vrc_box_words.h"
#include "vrc_group.h"

namespace {

constexpr uint32_t MAX_GROUPS = 16384;

inline uint32_t groups_for(uint64_t lanes)
{
    const uint64_t groups = (lanes + 255u) / 256u;
    return groups > MAX_GROUPS ? MAX_GROUPS : (uint32_t)groups;
}

// the count of cell (X, Y, Z) of level K = 1, 2, 3 in registers; lgs = log2 of the source's bricks per axis (K <= lgs + 1)
template <int K>
__device__ __forceinline__ uint32_t small_count(const uint32_t* __restrict__ src, uint32_t lgs, uint32_t X, uint32_t Y, uint32_t Z)
{
    constexpr uint32_t C = 1u << (K - 1);
    uint32_t sum = 0u;
#pragma unroll
    for (uint32_t i = 0; i < C; ++i)
#pragma unroll
        for (uint32_t j = 0; j < C; ++j) {
            const uint32_t byte = ((((X * C + i) << lgs) | (Y * C + j)) << lgs) + Z * C;       // below 2^27; a multiple of C
            if (K == 1) sum += (uint32_t)__popc(((const uint8_t*)src)[byte]);
            else if (K == 2) sum += (uint32_t)__popc(((const uint16_t*)src)[byte >> 1]);
            else sum += (uint32_t)__popc(src[byte >> 2]);
        }
    return sum;
}

// k = 1: a lane per source word, whose four bytes are four consecutive counts
__global__ __launch_bounds__(256) void k_counts_bytes(const uint32_t* __restrict__ src, uint32_t n_words, uint32_t* __restrict__ counts)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_words; i += gridDim.x * 256u) {
        const uint32_t w = src[i];
        uint32_t* out = counts + 4ull * i;
        out[0] = (uint32_t)__popc(w & 0xffu);
        out[1] = (uint32_t)__popc(w & 0xff00u);
        out[2] = (uint32_t)__popc(w & 0xff0000u);
        out[3] = (uint32_t)__popc(w & 0xff000000u);
    }
}

// k = 2, 3: a lane per cell in the dense order; lc = log2 of the cells per axis
template <int K>
__global__ __launch_bounds__(256) void k_counts_small(const uint32_t* __restrict__ src, uint32_t lgs, uint32_t lc, uint32_t* __restrict__ counts)
{
    const uint32_t n_cells = 1u << (3u * lc), m = (1u << lc) - 1u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_cells; i += gridDim.x * 256u)
        counts[i] = small_count<K>(src, lgs, i >> (2u * lc), (i >> lc) & m, i & m);
}

// k >= 4: unit u = (cell, part) = (u >> lgp, u & (2^lgp - 1)), a workgroup per unit; a part is LEVELS_GROUP_WORDS words of the
// cell's 2^(3 lgc - 2), numbered along the cell's brick rows.  lgc = k - 1 = log2 of the cell's bricks per axis, >= 3.
__global__ __launch_bounds__(256) void k_counts_large(const uint32_t* __restrict__ src, uint32_t lgs, uint32_t lgc, uint32_t lc, uint32_t lgp,
                                                      uint32_t* __restrict__ counts)
{
    __shared__ uint32_t part_sums[4];
    const uint32_t lgw = lgc - 2u, cell_words = 1u << (3u * lgc - 2u), m = (1u << lc) - 1u;
    const uint32_t units = 1u << (3u * lc + lgp);
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {                 // the same trip count for the whole group
        const uint32_t cell = u >> lgp, part = u & ((1u << lgp) - 1u);
        const uint32_t X = cell >> (2u * lc), Y = (cell >> lc) & m, Z = cell & m;
        uint32_t sum = 0u;
#pragma unroll
        for (uint32_t j = 0; j < vrc::LEVELS_GROUP_WORDS / 256u; ++j) {
            const uint32_t it = part * vrc::LEVELS_GROUP_WORDS + j * 256u + threadIdx.x;
            if (it >= cell_words) break;
            const uint32_t row = it >> lgw, wi = it & ((1u << lgw) - 1u);
            const uint32_t bx = (X << lgc) + (row >> lgc), by = (Y << lgc) + (row & ((1u << lgc) - 1u));
            sum += (uint32_t)__popc(src[(((bx << lgs) | by) << (lgs - 2u)) + (Z << lgw) + wi]);
        }
        const uint32_t all = group_sum<4u>(sum, part_sums);                    // at most 2048 * 32
        if (threadIdx.x == 0) {
            if (lgp == 0u) counts[cell] = all;
            else if (all) atomicAdd(&counts[cell], all);
        }
    }
}

// k = 1 into a field of 8^3 and more: a lane per dst word; bit c of `table` says that a count of c is in the band.  lgd = log2
// of the destination's bricks per axis, >= 2; the source has 2^(lgd + 1), so a row's eight bytes are aligned.
__global__ __launch_bounds__(256) void k_reduce_bytes(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t lgd, uint32_t table, int op)
{
    const uint32_t lgz = lgd - 2u, lgs = lgd + 1u, n_words = 1u << (3u * lgd - 2u);
    for (uint32_t W = blockIdx.x * 256u + threadIdx.x; W < n_words; W += gridDim.x * 256u) {
        const uint32_t cx = W >> (lgz + lgd), cy = (W >> lgz) & ((1u << lgd) - 1u), wz = W & ((1u << lgz) - 1u);
        uint32_t K = 0u;
#pragma unroll
        for (uint32_t r = 0; r < 4u; ++r) {                                    // r = yb * 2 + xb as in a word's bit index
            const uint32_t byte = ((((2u * cx + (r & 1u)) << lgs) | (2u * cy + (r >> 1))) << lgs) + 8u * wz;
            const uint2 v = ((const uint2*)src)[byte >> 3];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                K |= ((table >> __popc((v.x >> (8u * j)) & 0xffu)) & 1u) << (4u * j + r);
                K |= ((table >> __popc((v.y >> (8u * j)) & 0xffu)) & 1u) << (4u * (j + 4u) + r);
            }
        }
        store_selected_word(dst, W, K, op);
    }
}

// A lane per dst voxel: lane i is bit i & 31 of word i >> 5.  K = 1, 2, 3: the cell is counted here; K = 0: its count is read
// from `counts`, dense over the destination.  The voxels are a multiple of 64, so a wave is in the loop as a whole.
template <int K>
__global__ __launch_bounds__(256) void k_reduce_voxels(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, const uint32_t* __restrict__ counts,
                                                       uint32_t lgs, uint32_t lgd, uint32_t lo, uint32_t hi, int op)
{
    const uint32_t n_voxels = 8u << (3u * lgd), ld = lgd + 1u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_voxels; i += gridDim.x * 256u) {
        const uint32_t W = i >> 5, bit = i & 31u;
        uint32_t cx, cy, Z;
        if (lgd >= 2u) {
            const uint32_t lgz = lgd - 2u;
            cx = W >> (lgz + lgd); cy = (W >> lgz) & ((1u << lgd) - 1u); Z = 8u * (W & ((1u << lgz) - 1u)) + (bit >> 2);
        } else {
            cx = W; cy = bit >> 4; Z = (bit >> 2) & 3u;                        // 4^3: word cx, half cy
        }
        const uint32_t X = 2u * cx + (bit & 1u), Y = 2u * cy + ((bit >> 1) & 1u);
        const uint32_t count = K ? small_count<(K ? K : 1)>(src, lgs, X, Y, Z) : counts[(((X << ld) | Y) << ld) | Z];
        const unsigned long long in_band = __ballot(count >= lo && count < hi);
        if (bit == 0u) store_selected_word(dst, W, (uint32_t)(in_band >> (threadIdx.x & 32u)), op);
    }
}

// A lane per dst word; lgd = log2 of the destination's bricks per axis, >= 2, the source has 2^(lgd - k)
__global__ __launch_bounds__(256) void k_expand(uint32_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t lgd, uint32_t k, int op)
{
    const uint32_t lgz = lgd - 2u, lgs = lgd - k, n_words = 1u << (3u * lgd - 2u), down = k - 1u;
    for (uint32_t W = blockIdx.x * 256u + threadIdx.x; W < n_words; W += gridDim.x * 256u) {
        const uint32_t cx = W >> (lgz + lgd), cy = (W >> lgz) & ((1u << lgd) - 1u), wz = W & ((1u << lgz) - 1u);
        const uint32_t sx = cx >> down, sy = cy >> down;                       // the source voxel of the bricks (cx, cy, .)
        const uint32_t row = (((sx >> 1) << lgs) | (sy >> 1)) << lgs, xy_bit = (sy & 1u) * 2u + (sx & 1u);
        uint32_t K = 0u, brick = 0u, loaded = 0xffffffffu;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t sz = (4u * wz + j) >> down;
            if ((sz >> 1) != loaded) { loaded = sz >> 1; brick = src[row + loaded]; }
            if ((brick >> (xy_bit + 4u * (sz & 1u))) & 1u) K |= 0xffu << (8u * j);
        }
        store_selected_word(dst, W, K, op);
    }
}

}  // namespace

namespace vrc {

hipError_t levels_counts_run(const uint32_t* src, uint32_t depth, uint32_t k, uint32_t* counts, hipStream_t st)
{
    const uint32_t lgs = depth - 1u, lc = depth - k;
    if (k == 1u) {
        const uint32_t n_words = 1u << (3u * lgs - 2u);
        hipLaunchKernelGGL(k_counts_bytes, dim3(groups_for(n_words)), dim3(256), 0, st, src, n_words, counts);
    } else if (k == 2u) {
        hipLaunchKernelGGL(k_counts_small<2>, dim3(groups_for(1ull << (3u * lc))), dim3(256), 0, st, src, lgs, lc, counts);
    } else if (k == 3u) {
        hipLaunchKernelGGL(k_counts_small<3>, dim3(groups_for(1ull << (3u * lc))), dim3(256), 0, st, src, lgs, lc, counts);
    } else {
        // 2^(3 k - 5) words in a cell, 2^11 to a part
        const uint32_t lgp = 3u * k > 16u ? 3u * k - 16u : 0u;
        if (lgp) {
            const hipError_t e = hipMemsetAsync(counts, 0, (size_t)4u << (3u * lc), st);
            if (e != hipSuccess) return e;
        }
        const uint64_t units = 1ull << (3u * lc + lgp);                        // at most 2^18 (k = 4 at depth 10)
        hipLaunchKernelGGL(k_counts_large, dim3(units > MAX_GROUPS ? MAX_GROUPS : (uint32_t)units), dim3(256), 0, st, src, lgs, k - 1u, lc, lgp, counts);
    }
    return hipSuccess;
}

size_t levels_scratch_bytes(uint32_t src_depth, uint32_t k) { return k < 4u ? 0u : (size_t)4u << (3u * (src_depth - k)); }

hipError_t levels_reduce_run(uint32_t* dst, const uint32_t* src, uint32_t src_depth, uint32_t k, uint32_t lo, uint32_t hi, int op, uint32_t* scratch,
                             hipStream_t st)
{
    const uint32_t lgs = src_depth - 1u, lgd = src_depth - k - 1u;
    const uint32_t groups = groups_for(8ull << (3u * lgd));
    if (k == 1u && lgd >= 2u) {
        uint32_t table = 0u;
        for (uint32_t c = 0; c <= 8u; ++c)
            if (c >= lo && c < hi) table |= 1u << c;
        hipLaunchKernelGGL(k_reduce_bytes, dim3(groups_for(1ull << (3u * lgd - 2u))), dim3(256), 0, st, dst, src, lgd, table, op);
    } else if (k == 1u) {
        hipLaunchKernelGGL(k_reduce_voxels<1>, dim3(groups), dim3(256), 0, st, dst, src, (const uint32_t*)nullptr, lgs, lgd, lo, hi, op);
    } else if (k == 2u) {
        hipLaunchKernelGGL(k_reduce_voxels<2>, dim3(groups), dim3(256), 0, st, dst, src, (const uint32_t*)nullptr, lgs, lgd, lo, hi, op);
    } else if (k == 3u) {
        hipLaunchKernelGGL(k_reduce_voxels<3>, dim3(groups), dim3(256), 0, st, dst, src, (const uint32_t*)nullptr, lgs, lgd, lo, hi, op);
    } else {
        const hipError_t e = levels_counts_run(src, src_depth, k, scratch, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_reduce_voxels<0>, dim3(groups), dim3(256), 0, st, dst, src, (const uint32_t*)scratch, lgs, lgd, lo, hi, op);
    }
    return hipSuccess;
}

void levels_expand_run(uint32_t* dst, uint32_t dst_depth, const uint32_t* src, uint32_t k, int op, hipStream_t st)
{
    const uint32_t lgd = dst_depth - 1u;
    hipLaunchKernelGGL(k_expand, dim3(groups_for(1ull << (3u * lgd - 2u))), dim3(256), 0, st, dst, (const uint8_t*)src, lgd, k, op);
}

}  // namespace vrc
