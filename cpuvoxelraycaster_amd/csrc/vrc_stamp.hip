// vrc_stamp.hip -- stamping one voxel volume into another through an affine map, exact in integers (include/vrc.h:
// vrc_volume_stamp_affine): rotated, mirrored and scaled pastes without leaving the device.  The map is the INVERSE map --
// it says where each destination voxel reads from -- so every destination voxel of the box is written from exactly one
// source voxel and a rotation leaves no holes.
//
// Work layout: vrc_volume.hip's region copy.  One thread per destination occupancy word of the box's brick rows
// (vrc_box_words.h; a word = four bricks along z = 2 x 2 x 8 voxels); it gathers the word's 32 source bits and writes the
// word once, a partly covered word as a masked read-modify-write -- a word has one owner within a call, except in volumes
// of 4^3, where two rows share a word and take 32-bit vector atomics.
//
// Arithmetic: s = m (2p + 1) + t is 64-bit (|s| < 2^41) and is evaluated ONCE per word, for the word's first voxel, and
// split into q_base = s >> 17 and frac = s & 0x1ffff.  Every other voxel of the word is q_base + ((frac + delta) >> 17)
// with delta = 2 (i m_x + j m_y + k m_z), i, j < 2, k < 8: below 2^25 in magnitude with |m| <= 2^20, so 32-bit signed, and
// a running sum along the column.  The smallest and the largest delta per source axis give the word's bounding box in the
// source: a box that misses the source on any axis makes the word's bits 0 without a load (an OR / ANDNOT word is then
// left alone), and one wholly inside drops the per-voxel bounds tests.
#include "vrc_stamp.h"

#include "vrc_box_words.h"

namespace {

// The 32 source bits of one destination word, under `mask`.  q[a] / frac[a]: source coordinate and 17-bit fraction of the
// word's first voxel; step[a][c]: what one voxel along destination axis c adds to s_a.  Successive voxels of a column
// often fall into the same source brick (always, in pairs, at scale 1 without a turn about x or y): its byte is kept.
template <bool INSIDE>
__device__ __forceinline__ uint32_t gather_word(const uint8_t* __restrict__ src, uint32_t ns, const int32_t q[3], const int32_t frac[3],
                                                const int32_t step[3][3], uint32_t mask)
{
    const uint32_t Ss = 2u * ns;
    uint32_t bits = 0u, last = 0xffffffffu, byte = 0u;
#pragma unroll
    for (uint32_t col = 0; col < 4u; ++col) {          // col = y * 2 + x, as in a brick's bit index
        int32_t d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = frac[a] + ((col & 1u) ? step[a][0] : 0) + ((col & 2u) ? step[a][1] : 0);
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const uint32_t bit = (k >> 1) * 8u + (k & 1u) * 4u + col;
            if ((mask >> bit) & 1u) {
                const uint32_t x = (uint32_t)(q[0] + (d[0] >> 17)), y = (uint32_t)(q[1] + (d[1] >> 17)), z = (uint32_t)(q[2] + (d[2] >> 17));
                if (INSIDE || (x < Ss && y < Ss && z < Ss)) {          // unsigned: a negative coordinate is a large one
                    const uint32_t at = ((x >> 1) * ns + (y >> 1)) * ns + (z >> 1);     // < 2^27
                    if (at != last) { last = at; byte = src[at]; }
                    bits |= ((byte >> voxel_bit(x, y, z)) & 1u) << bit;
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) d[a] += step[a][2];
        }
    }
    return bits;
}

__global__ void __launch_bounds__(256) k_stamp_affine(uint32_t* __restrict__ dst, uint32_t Sd, const uint8_t* __restrict__ src, uint32_t Ss, vrc_affine map,
                                                      uint32_t lx, uint32_t ly, uint32_t lz, uint32_t hx, uint32_t hy, uint32_t hz, int op)
{
    const uint32_t lo[3] = {lx, ly, lz}, hi[3] = {hx, hy, hz};
    const uint32_t n = Sd >> 1, ns = Ss >> 1;
    const BoxWords b = box_words(lo, hi);
    // per source axis: s per destination voxel step (|.| <= 2^21), and the extremes of delta over a word's 2 x 2 x 8 voxels
    int32_t step[3][3], dmin[3], dmax[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) step[a][c] = 2 * map.m[3 * a + c];
        dmin[a] = min(step[a][0], 0) + min(step[a][1], 0) + 7 * min(step[a][2], 0);
        dmax[a] = max(step[a][0], 0) + max(step[a][1], 0) + 7 * max(step[a][2], 0);
    }
    for (uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < b.items; it += (uint64_t)gridDim.x * blockDim.x) {
        RowWord r;
        if (!row_word(b, n, it, r)) continue;
        const uint32_t mask = box_mask(b, r);
        if (!mask) continue;
        // z of the word's first voxel, relative to the row (negative where the word starts in the row before: n = 2; those
        // voxels are outside the mask)
        const int64_t z0 = 2 * ((int64_t)(4u * r.w) - (int64_t)r.base);
        const int64_t c[3] = {4 * (int64_t)r.cx + 1, 4 * (int64_t)r.cy + 1, 2 * z0 + 1};       // 2p + 1: the centre in half voxels
        int32_t q[3], frac[3];
        bool miss = false, inside = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int64_t s = (int64_t)map.m[3 * a] * c[0] + (int64_t)map.m[3 * a + 1] * c[1] + (int64_t)map.m[3 * a + 2] * c[2] + map.t[a];
            q[a] = (int32_t)(s >> 17);                 // |s| < 2^41
            frac[a] = (int32_t)(s & 0x1ffff);
            const int32_t qmin = q[a] + ((frac[a] + dmin[a]) >> 17), qmax = q[a] + ((frac[a] + dmax[a]) >> 17);
            miss = miss || qmax < 0 || qmin >= (int32_t)Ss;
            inside = inside && qmin >= 0 && qmax < (int32_t)Ss;
        }
        uint32_t bits = 0u;
        if (miss) { if (op != VRC_COPY_REPLACE) continue; }
        else bits = inside ? gather_word<true>(src, ns, q, frac, step, mask) : gather_word<false>(src, ns, q, frac, step, mask);
        store_box_word(dst, r.w, mask, bits, op, n < 4u);
    }
}

}  // namespace

namespace vrc {

void stamp_affine_run(uint32_t* dst, uint32_t dst_depth, const uint32_t* src, uint32_t src_depth, const vrc_affine& map, const uint32_t lo[3],
                      const uint32_t hi[3], int op, hipStream_t st)
{
    hipLaunchKernelGGL(k_stamp_affine, dim3(box_launch_groups(lo, hi)), dim3(256), 0, st, dst, 1u << dst_depth, (const uint8_t*)src, 1u << src_depth, map,
                       lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], op);
}

}  // namespace vrc
