// vrc_voxelize.hip -- solid voxelisation of triangle meshes by crossing parity along z (include/vrc.h:
// vrc_volume_xor_mesh; the scheme of Schwarz & Seidel, "Fast parallel surface and solid voxelization on GPUs", 2010).
//
// The occupancy is one byte per 2 x 2 x 2 brick, four bricks along z per 32-bit word: a word is 2 x 2 x 8 voxels, bit
// zz*4 + yb*2 + xb -- eight z layers of one nibble -- and the words of a brick column (cx, cy) are contiguous along z.
// A triangle flips, in every voxel column whose centre its xy projection covers, the voxels whose centres lie below its
// plane: a prefix [0, k) of the column.  Two passes on one stream:
//   * mark: blockIdx.x = triangle, its work -- the columns of its xy bounding box clipped to the volume -- split over
//     blockIdx.y x blockDim.x threads.  A covered column with k >= 1 toggles ONE bit, voxel k - 1 of the column, in a mark
//     field with the occupancy's layout: a 32-bit vector atomicXor, so that a second crossing at the same voxel cancels
//     the first.  Few triangles are spread over up to 1024 workgroups each; more than 4096 get one workgroup each
//     whatever their size, so thousands of roof-sized triangles in one call each walk their bounding box on four waves.
//   * scan: the flips of a column are the inclusive suffix XOR of its marks along z.  One lane per word (two words at
//     depth 10), a column's words on neighbouring lanes of one wave: within a word the suffix is three shifts
//     (w ^= w >> 4, >> 8, >> 16), across the words a 4-bit carry -- one bit per (x, y) of the brick -- scanned over the
//     column's lanes.  The result is XORed into the occupancy word where it is non-zero, and every mark word read
//     non-zero is stored back as 0: the field is all zero again when the pass ends.  A wave without a mark leaves after
//     its loads.  A word has one owner, so plain loads and stores.  The grid covers the WHOLE field whatever the mesh's
//     size: a call costs at least one read of the mark field (16 MiB at 512^3, 128 MiB at 1024^3), so a small model
//     goes through a small clipboard volume and vrc_volume_copy_region (VoxelVolume.stampMesh), not into the world
//     directly.  Restricting the grid to the batch's brick-column bounding box would lift that floor; not done.
// XOR commutes and every quantity is an integer: the result does not depend on scheduling or on the triangles' order.
// All arithmetic is int64; with |coordinate| <= 2^17 every product and sum stays below 2^57 (include/vrc.h).
#include "vrc_voxelize.h"

namespace {

constexpr int32_t MESH_LIMIT = 1 << 17;        // |coordinate| in 1/64 voxel; include/vrc.h: VRC_MESH_FRAC_BITS

__global__ void k_mark_triangles(uint32_t* __restrict__ marks, uint32_t S, const int32_t* __restrict__ tris)
{
    const int32_t* t = tris + 9ull * blockIdx.x;
    int64_t v[9];
    for (int i = 0; i < 9; ++i) {
        const int32_t c = t[i];
        if (c > MESH_LIMIT || c < -MESH_LIMIT) return;                 // uniform for the workgroup, as every return below
        v[i] = c;
    }
    const int64_t ax = v[0], ay = v[1], az = v[2];
    const int64_t ux = v[3] - ax, uy = v[4] - ay, uz = v[5] - az, wx = v[6] - ax, wy = v[7] - ay, wz = v[8] - az;
    const int64_t nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    if (nz == 0) return;
    const int64_t s = nz > 0 ? 1 : -1, anz = nz > 0 ? nz : -nz;
    // the columns whose centres 64 c + 32 lie in the xy bounding box, clipped to the volume
    int64_t lo[2], hi[2];
    for (int a = 0; a < 2; ++a) {
        int64_t mn = v[a], mx = v[a];
        for (int k = 1; k < 3; ++k) {
            mn = v[3 * k + a] < mn ? v[3 * k + a] : mn;
            mx = v[3 * k + a] > mx ? v[3 * k + a] : mx;
        }
        lo[a] = (mn + 31) >> 6;                                        // ceil((mn - 32) / 64)
        hi[a] = (mx - 32) >> 6;                                        // floor((mx - 32) / 64)
        if (lo[a] < 0) lo[a] = 0;
        if (hi[a] > (int64_t)S - 1) hi[a] = (int64_t)S - 1;
        if (lo[a] > hi[a]) return;
    }
    // edges P -> Q oriented by s: the interior is on the left of each
    int64_t px0[3], py0[3], dx[3], dy[3];
    bool tie[3];
    for (int e = 0; e < 3; ++e) {
        const int p = 3 * e, q = 3 * ((e + 1) % 3);
        px0[e] = v[p]; py0[e] = v[p + 1];
        dx[e] = s * (v[q] - v[p]); dy[e] = s * (v[q + 1] - v[p + 1]);
        tie[e] = dy[e] > 0 || (dy[e] == 0 && dx[e] < 0);
    }
    const uint32_t ncy = (uint32_t)(hi[1] - lo[1] + 1);
    const uint32_t items = (uint32_t)(hi[0] - lo[0] + 1) * ncy;        // at most 2^20
    const uint32_t n = S >> 1;
    const int64_t D = 64 * anz;
    for (uint32_t it = blockIdx.y * blockDim.x + threadIdx.x; it < items; it += gridDim.y * blockDim.x) {
        const uint32_t x = (uint32_t)lo[0] + it / ncy, y = (uint32_t)lo[1] + it % ncy;
        const int64_t px = 64 * (int64_t)x + 32, py = 64 * (int64_t)y + 32;
        bool covered = true;
        for (int e = 0; e < 3; ++e) {
            const int64_t E = dx[e] * (py - py0[e]) - dy[e] * (px - px0[e]);
            covered = covered && (E > 0 || (E == 0 && tie[e]));
        }
        if (!covered) continue;
        const int64_t N = anz * (az - 32) - s * (nx * (px - ax) + ny * (py - ay));
        if (N <= 0) continue;                                          // k = 0: the plane passes below the column
        const uint32_t k = N > (int64_t)(S - 1u) * D ? S : (uint32_t)((N + D - 1) / D);
        const uint32_t z = k - 1u;
        const uint64_t brick = ((uint64_t)(x >> 1) * n + (y >> 1)) * n + (z >> 1);
        atomicXor(&marks[brick >> 2], 1u << (((z & 1u) * 4u + (y & 1u) * 2u + (x & 1u)) + 8u * (uint32_t)(brick & 3u)));
    }
}

// nibble j of the result = XOR of the nibbles j.. of w
__device__ __forceinline__ uint32_t suffix_xor(uint32_t w)
{
    w ^= w >> 4; w ^= w >> 8; w ^= w >> 16;
    return w;
}

// lanes = lanes per brick column (a power of two, at most 64), PER = words per lane (1, or 2 at depth 10).  Lane i owns
// words [i * PER, i * PER + PER); columns never straddle a wave.
template <uint32_t PER>
__global__ void k_scan_columns(uint32_t* __restrict__ occupancy, uint32_t* __restrict__ marks, uint64_t n_words, uint32_t lanes)
{
    const uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * PER;
    const bool valid = w < n_words;
    uint32_t m[PER], f[PER];
    uint32_t own = 0u, any = 0u;
    for (uint32_t j = 0; j < PER; ++j) {
        m[j] = valid ? marks[w + j] : 0u;
        f[j] = suffix_xor(m[j]);
        own ^= f[j] & 0xfu;                                            // XOR of all nibbles of this lane's words
        any |= m[j];
    }
    if (__ballot(any != 0u) == 0ull) return;                           // no mark in this wave's columns
    // XOR of `own` over this and the higher lanes of the column
    const uint32_t pos = threadIdx.x & (lanes - 1u);
    uint32_t incl = own;
    for (uint32_t d = 1u; d < lanes; d <<= 1) {
        const uint32_t other = (uint32_t)__shfl_down((int)incl, d);
        if (pos + d < lanes) incl ^= other;
    }
    uint32_t carry = incl ^ own;                                       // from the words above this lane's
    for (uint32_t j = PER; j-- > 0u;) {
        const uint32_t flips = f[j] ^ (carry * 0x11111111u);
        carry = flips & 0xfu;
        if (m[j]) marks[w + j] = 0u;
        if (flips) occupancy[w + j] ^= flips;
    }
}

// 4^3: a brick column is two bytes, half a word, and two columns share a word: one thread per column, atomics
__global__ void k_scan_columns_4(uint32_t* __restrict__ occupancy, uint32_t* __restrict__ marks)
{
    const uint32_t base = 2u * threadIdx.x;                            // byte of brick (cx, cy, 0), threadIdx.x = cx * 2 + cy
    const uint32_t word = base >> 2, shift = 8u * (base & 3u);
    const uint32_t m = (marks[word] >> shift) & 0xffffu;
    if (!m) return;
    uint32_t f = m;
    f ^= f >> 4; f ^= f >> 8;
    atomicXor(&marks[word], m << shift);                               // this half back to zero
    atomicXor(&occupancy[word], f << shift);
}

}  // namespace

namespace vrc {

size_t voxelize_scratch_bytes(uint32_t depth) { return (size_t)1 << (3u * (depth - 1u)); }

void voxelize_run(uint32_t* occupancy, uint32_t* marks, uint32_t depth, uint64_t n, const int32_t* tris, hipStream_t st)
{
    const uint32_t S = 1u << depth;
    const uint64_t n_words = ((uint64_t)1 << (3u * (depth - 1u))) / 4u;
    // workgroups per triangle: 256-thread groups that cover the largest possible bounding box (S^2 columns) once at most.
    // The rule of split_for in vrc_volume.hip (4096 workgroups in all, at most 1024 per item) with columns for its words:
    // keep the two in step.
    uint32_t split = (uint32_t)((4096ull + n - 1) / n);
    const uint32_t useful = (S * S + 255u) / 256u;
    if (split > 1024u) split = 1024u;
    if (split > useful) split = useful;
    hipLaunchKernelGGL(k_mark_triangles, dim3((uint32_t)n, split), dim3(256), 0, st, marks, S, tris);
    if (depth == 2u) {
        hipLaunchKernelGGL(k_scan_columns_4, dim3(1), dim3(4), 0, st, occupancy, marks);
        return;
    }
    const uint32_t column_words = S >> 3;                              // 1 .. 128
    if (column_words <= 64u) {
        hipLaunchKernelGGL(k_scan_columns<1>, dim3((uint32_t)((n_words + 255u) / 256u)), dim3(256), 0, st, occupancy, marks, n_words, column_words);
    } else {
        hipLaunchKernelGGL(k_scan_columns<2>, dim3((uint32_t)((n_words / 2u + 255u) / 256u)), dim3(256), 0, st, occupancy, marks, n_words, 64u);
    }
}

}  // namespace vrc
