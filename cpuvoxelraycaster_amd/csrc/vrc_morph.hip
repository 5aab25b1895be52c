// vrc_morph.hip -- dilation and erosion of the occupancy field by a structuring element of the caller's choice
// (include/vrc.h: vrc_morph_apply): the Minkowski sum and difference with a box, a line, a cross, a ball or a piece's own
// voxels, where vrc_cells.hip reaches one voxel and vrc_distance.hip knows the ball alone.
//
// The layout of a word (2 x 2 x 8 voxels, bit zz*4 + yb*2 + xb) is described at the top of vrc_flood.hip; the words of a
// brick row are consecutive along z.
//
// One loop for all four forms.  With A' = A for DILATE and its complement for ERODE (beyond the faces included), and
// E' = E for DILATE and -E for ERODE,
//     K'(p) = OR over e in E' of A'(p - e),        K = K' for DILATE and its complement for ERODE,
// because AND over e of A(p + e) is the complement of OR over e of not-A(p + e).  `of` EMPTY is one more complement on load.
// So the kernels take three masks (cin: xor on load, edge: what lies beyond the faces after it, cout: xor on store) and the
// sign the list is read with.
//
// Prepare.  k_morph_prepare, a lane per offset: e = sign * (offset - origin) in 64 bits, dropped when a component is beyond
// +-16, else one 64-bit atomicOr of bit ez + 16 into the z mask of column (ex + 16, ey + 16) of a 33 x 33 table zeroed on the
// stream before it.  Duplicates fall together there.  k_morph_compact, one workgroup: the non-empty columns as a list, their
// number and the element's box.  The apply's work follows that list and the set bits of its masks, neither n nor the 33^3 cube.
//
// Apply.  A workgroup owns 16 x 16 brick columns (32 x 32 voxel columns) and 32 voxels of z; a lane owns one brick column of
// it, that is four words consecutive along z, which it stores once -- as one 16-byte store from 32^3 on.  The source goes
// into LDS as PILLARS: per voxel column (x, y) of the tile and of the halo the element's box asks for, the 64 z bits
// [z0 - 16, z0 + 48), transposed out of the words with column_bits_of_word by a lane per brick column of the region, the
// complement and the faces applied there.  In that form a step along x or y is an index, whatever its parity, and a step
// along z a shift: the 32 result bits of a pillar for the offset (ex, ey, ez) are  pillar(x - ex, y - ey) >> (16 - ez).  Per
// column of the list a lane reads its four pillars once and ORs one shifted copy per set bit of the mask; the list and the
// masks are uniform over the workgroup, so the two loops are scalar.  Four results are transposed back into words.
// Why not the suggested tile sized from the box: with the list in device memory only the device knows the box, and the host
// does not wait for it.  So the LDS block is the largest one, 64 x 64 pillars in two parity planes of pitch 40, 40 KiB and four
// workgroups a CU, and it is the staging WORK that follows the box: (32 + wx) x (32 + wy) pillars, and of their eight words only
// those that the z extent reaches.  The planes split y by parity, so that the 16 lanes of a row read consecutive 8 bytes,
// and the pitch is 8 mod 16, so that the next brick column of x lands on the other half of the banks.
// 4^3: a word holds the brick rows cy = 0, 1 of one cx, 16 bits each; the halves are read as words whose z layers 4 .. 7 lie
// beyond the face, and the lane of cy = 0 takes the other half from its neighbour lane and stores the whole word.
// Every index into the table and into LDS is clamped to the table and the box before use, whatever the block holds; no trip
// count depends on anything but n, the tile and the element.
#include "vrc_morph.h"

#include "../../include/vrc.h"
#include "vrc_word_columns.h"

namespace {

constexpr int32_t REACH = VRC_MORPH_REACH;
constexpr uint32_t MASK_BYTES = vrc::MORPH_COLUMNS * 8u;
constexpr uint32_t TILE = 16u;                       // brick columns per axis of a workgroup's tile
constexpr uint32_t PILLARS = 2u * 64u * 40u;         // two parity planes, 64 rows, the larger pitch

struct Header {
    uint32_t count;
    int32_t x0, x1, y0, y1, z0, z1;
    uint32_t zero;
};
static_assert(MASK_BYTES + sizeof(Header) + vrc::MORPH_COLUMNS * 4u <= vrc::MORPH_BLOCK_BYTES, "the prepared element fits its block");
static_assert(REACH == 16 && vrc::MORPH_SIDE == 2u * REACH + 1u, "a z mask is 33 bits of a 64-bit word");

__device__ __forceinline__ int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// a lane per offset; the masks are zero before the launch
__global__ __launch_bounds__(256) void k_morph_prepare(unsigned long long* __restrict__ mask, const int32_t* __restrict__ offsets, uint64_t n, int32_t ox,
                                                       int32_t oy, int32_t oz, int32_t sign)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int64_t ex = ((int64_t)offsets[3u * i] - ox) * sign, ey = ((int64_t)offsets[3u * i + 1u] - oy) * sign, ez = ((int64_t)offsets[3u * i + 2u] - oz) * sign;
    if (ex < -REACH || ex > REACH || ey < -REACH || ey > REACH || ez < -REACH || ez > REACH) return;
    atomicOr(&mask[(uint32_t)(ex + REACH) * vrc::MORPH_SIDE + (uint32_t)(ey + REACH)], 1ull << (uint32_t)(ez + REACH));
}

// one workgroup: the list of the non-empty columns and the box
__global__ __launch_bounds__(256) void k_morph_compact(const unsigned long long* __restrict__ mask, Header* __restrict__ header, uint32_t* __restrict__ cols)
{
    __shared__ uint32_t count;
    __shared__ int32_t box[4];
    __shared__ unsigned long long layers;
    if (threadIdx.x == 0) {
        count = 0u; layers = 0ull;
        box[0] = box[2] = REACH; box[1] = box[3] = -REACH;
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < vrc::MORPH_COLUMNS; c += 256u) {
        const unsigned long long m = mask[c];
        if (!m) continue;
        const uint32_t ix = c / vrc::MORPH_SIDE, iy = c - ix * vrc::MORPH_SIDE;
        cols[atomicAdd(&count, 1u)] = ix | (iy << 8);                  // at most MORPH_COLUMNS of them
        atomicMin(&box[0], (int32_t)ix - REACH); atomicMax(&box[1], (int32_t)ix - REACH);
        atomicMin(&box[2], (int32_t)iy - REACH); atomicMax(&box[3], (int32_t)iy - REACH);
        atomicOr(&layers, m);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    Header h = {count, 0, 0, 0, 0, 0, 0, 0u};
    if (count) {
        h.x0 = box[0]; h.x1 = box[1]; h.y0 = box[2]; h.y1 = box[3];
        h.z0 = (int32_t)__builtin_ctzll(layers) - REACH;
        h.z1 = 63 - (int32_t)__builtin_clzll(layers) - REACH;
    }
    *header = h;
}

// the 8 bits of b to bit 4 * i each: the inverse of column_bits_of_word at sh = 0
__device__ __forceinline__ uint32_t spread_bits(uint32_t b)
{
    uint32_t t = (b | (b << 12)) & 0x000f000fu;
    t = (t | (t << 6)) & 0x03030303u;
    return (t | (t << 3)) & 0x11111111u;
}

// the word whose voxel columns q = yb * 2 + xb hold byte k of r[q]
__device__ __forceinline__ uint32_t word_of_pillars(const uint32_t r[4], uint32_t k)
{
    uint32_t w = 0u;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) w |= spread_bits((r[q] >> (8u * k)) & 0xffu) << q;
    return w;
}

__device__ __forceinline__ uint32_t under_op(uint32_t old, uint32_t bits, int op)
{
    return op == VRC_COPY_REPLACE ? bits : op == VRC_COPY_OR ? (old | bits) : (old & ~bits);
}

// blockIdx: x the tile along y, y the tile along x, z the 32 voxels along z.  lg = log2 of the brick rows per axis.
template <bool SMALL>
__global__ __launch_bounds__(256) void k_morph_apply(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t lg,
                                                     const unsigned long long* __restrict__ mask, const Header* __restrict__ header,
                                                     const uint32_t* __restrict__ cols, uint32_t cin, uint32_t edge, uint32_t cout, int op)
{
    __shared__ unsigned long long pillars[PILLARS];
    const int32_t n = 1 << lg;
    const uint32_t lgz = SMALL ? 0u : lg - 2u;
    const int32_t nz = SMALL ? 1 : (n >> 2);                          // words of a brick row
    // the element: whatever the block holds, the box lies within the reach and is not inverted
    const uint32_t ncols = header->count < vrc::MORPH_COLUMNS ? header->count : vrc::MORPH_COLUMNS;
    const int32_t ax0 = clampi(header->x0, -REACH, REACH), ax1 = clampi(header->x1, ax0, REACH);
    const int32_t ay0 = clampi(header->y0, -REACH, REACH), ay1 = clampi(header->y1, ay0, REACH);
    const int32_t az0 = clampi(header->z0, -REACH, REACH), az1 = clampi(header->z1, az0, REACH);
    const unsigned long long layers = ((2ull << (uint32_t)(az1 + REACH)) - 1ull) & ~((1ull << (uint32_t)(az0 + REACH)) - 1ull);
    // the pillars held: lattice columns [sx0, sx0 + LX) x [sy0, sy0 + LY), LX, LY <= 64
    const int32_t LX = 2 * (int32_t)TILE + ax1 - ax0, LY = 2 * (int32_t)TILE + ay1 - ay0;
    const int32_t sx0 = (int32_t)(blockIdx.y * 2u * TILE) - ax1, sy0 = (int32_t)(blockIdx.x * 2u * TILE) - ay1;
    const int32_t pitch = LY <= 48 ? 24 : 40;
    auto at = [&](int32_t lx, int32_t ly) { return ((ly & 1) * LX + lx) * pitch + (ly >> 1); };    // below 128 * 40

    // ---- stage: a lane per brick column of the region; bit j of a pillar is z = 32 blockIdx.z - 16 + j, byte k word 4 blockIdx.z - 2 + k
    const int32_t bx0 = sx0 >> 1, by0 = sy0 >> 1;                     // floor, also below zero
    const int32_t nbx = ((sx0 + LX - 1) >> 1) - bx0 + 1, nby = ((sy0 + LY - 1) >> 1) - by0 + 1;      // at most 33
    const int32_t k_lo = (REACH - az1) >> 3, k_hi = (47 - az0) >> 3;  // the bytes that the z extent reaches, within 0 .. 7
    for (int32_t item = (int32_t)threadIdx.x; item < nbx * nby; item += 256) {
        const int32_t bi = item / nby, cx = bx0 + bi, cy = by0 + (item - bi * nby);
        unsigned long long pil[4] = {0ull, 0ull, 0ull, 0ull};
        if (cx < 0 || cy < 0 || cx >= n || cy >= n) {
            pil[0] = pil[1] = pil[2] = pil[3] = edge ? ~0ull : 0ull;
        } else {
#pragma unroll
            for (int32_t k = 0; k < 8; ++k) {
                if (k < k_lo || k > k_hi) continue;
                const int32_t wi = 4 * (int32_t)blockIdx.z - 2 + k;
                uint32_t w = edge;
                if (wi >= 0 && wi < nz) {
                    if (SMALL) w = (((src[cx] ^ cin) >> (16u * (uint32_t)cy)) & 0xffffu) | (edge << 16);
                    else w = src[((((uint32_t)cx << lg) + (uint32_t)cy) << lgz) + (uint32_t)wi] ^ cin;          // below 2^25
                }
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) pil[q] |= (unsigned long long)column_bits_of_word(w, q) << (8u * (uint32_t)k);
            }
        }
#pragma unroll
        for (int32_t q = 0; q < 4; ++q) {
            const int32_t lx = 2 * cx + (q & 1) - sx0, ly = 2 * cy + (q >> 1) - sy0;
            if (lx >= 0 && lx < LX && ly >= 0 && ly < LY) pillars[at(lx, ly)] = pil[q];
        }
    }
    __syncthreads();

    // ---- gather: the lane's four pillars, 32 bits each
    const int32_t cxl = (int32_t)(threadIdx.x >> 4), cyl = (int32_t)(threadIdx.x & 15u);
    uint32_t r[4] = {0u, 0u, 0u, 0u};
    for (uint32_t c = 0; c < ncols; ++c) {
        const uint32_t packed = cols[c];
        const uint32_t ix = (packed & 0xffu) < vrc::MORPH_SIDE ? (packed & 0xffu) : vrc::MORPH_SIDE - 1u;
        const uint32_t iy = ((packed >> 8) & 0xffu) < vrc::MORPH_SIDE ? ((packed >> 8) & 0xffu) : vrc::MORPH_SIDE - 1u;
        unsigned long long m = mask[ix * vrc::MORPH_SIDE + iy] & layers;
        const int32_t lx = 2 * cxl + ax1 - clampi((int32_t)ix - REACH, ax0, ax1), ly = 2 * cyl + ay1 - clampi((int32_t)iy - REACH, ay0, ay1);
        const unsigned long long v0 = pillars[at(lx, ly)], v1 = pillars[at(lx + 1, ly)], v2 = pillars[at(lx, ly + 1)], v3 = pillars[at(lx + 1, ly + 1)];
        while (m) {
            const uint32_t s = 2u * REACH - (uint32_t)__builtin_ctzll(m);                   // 16 - ez, 0 .. 32
            m &= m - 1ull;
            r[0] |= (uint32_t)(v0 >> s); r[1] |= (uint32_t)(v1 >> s); r[2] |= (uint32_t)(v2 >> s); r[3] |= (uint32_t)(v3 >> s);
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) r[q] ^= cout;

    // ---- store: every word of dst by its one owner
    const int32_t cx = (int32_t)(blockIdx.y * TILE) + cxl, cy = (int32_t)(blockIdx.x * TILE) + cyl;
    if (SMALL) {
        const uint32_t half = word_of_pillars(r, 0u) & 0xffffu;      // z = 0 .. 3
        const uint32_t other = (uint32_t)__shfl_down((int)half, 1);   // the lane of (cx, 1) is the next one
        if (cx < n && cy == 0) dst[cx] = under_op(dst[cx], half | (other << 16), op);
        return;
    }
    if (cx >= n || cy >= n) return;
    uint32_t* row = dst + ((((uint32_t)cx << lg) + (uint32_t)cy) << lgz) + 4u * blockIdx.z;
    if (nz >= 4) {
        uint4 old = make_uint4(0u, 0u, 0u, 0u);
        if (op != VRC_COPY_REPLACE) old = *(const uint4*)row;
        *(uint4*)row = make_uint4(under_op(old.x, word_of_pillars(r, 0u), op), under_op(old.y, word_of_pillars(r, 1u), op),
                                  under_op(old.z, word_of_pillars(r, 2u), op), under_op(old.w, word_of_pillars(r, 3u), op));
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < 2u; ++k)                                   // 8^3: one word, 16^3: two
        if ((int32_t)k < nz) row[k] = under_op(op != VRC_COPY_REPLACE ? row[k] : 0u, word_of_pillars(r, k), op);
}

}  // namespace

namespace vrc {

hipError_t morph_run(uint32_t* dst, const uint32_t* src, uint32_t depth, int erode, int of_empty, int outside, uint64_t n, const int32_t* d_offsets,
                     const int32_t origin[3], int op, void* d_block, hipStream_t st)
{
    unsigned long long* mask = (unsigned long long*)d_block;
    Header* header = (Header*)((uint8_t*)d_block + MASK_BYTES);
    uint32_t* cols = (uint32_t*)((uint8_t*)d_block + MASK_BYTES + sizeof(Header));
    const hipError_t e = hipMemsetAsync(mask, 0, MASK_BYTES, st);
    if (e != hipSuccess) return e;
    if (n) hipLaunchKernelGGL(k_morph_prepare, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, mask, d_offsets, n, origin[0], origin[1], origin[2], erode ? -1 : 1);
    hipLaunchKernelGGL(k_morph_compact, dim3(1), dim3(256), 0, st, mask, header, cols);
    const uint32_t cin = (of_empty != 0) != (erode != 0) ? 0xffffffffu : 0u, edge = (outside != 0) != (erode != 0) ? 0xffffffffu : 0u;
    const uint32_t cout = erode ? 0xffffffffu : 0u, lg = depth - 1u, S = 1u << depth;
    const uint32_t tiles = S > 2u * TILE ? S / (2u * TILE) : 1u;
    if (depth == 2u)
        hipLaunchKernelGGL(k_morph_apply<true>, dim3(1, 1, 1), dim3(256), 0, st, dst, src, lg, mask, header, cols, cin, edge, cout, op);
    else
        hipLaunchKernelGGL(k_morph_apply<false>, dim3(tiles, tiles, tiles), dim3(256), 0, st, dst, src, lg, mask, header, cols, cin, edge, cout, op);
    return hipSuccess;
}

}  // namespace vrc
