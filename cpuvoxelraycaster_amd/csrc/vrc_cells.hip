// vrc_cells.hip -- one step of a neighbour-count automaton on the occupancy field, and the seeded random fill of a box
// (include/vrc.h: vrc_cells_step, vrc_cells_fill_random): clean-up and smoothing by a vote of the neighbours, caves from a
// seed, any cellular rule.
//
// The layout of a word (2 x 2 x 8 voxels, bit zz*4 + yb*2 + xb) is described at the top of vrc_flood.hip, and the shifts
// are the flood's: a step along x is a shift by 1 under WORD_X0 / WORD_X1 with the other half from the word of the brick
// row next in x, along y by 2 under WORD_Y0 / WORD_Y1, along z by 4 with a nibble of the z-neighbour word.
//
// The step.  One lane owns one destination word and writes it once; the source is only read.  The lane brings the nine
// brick rows (cx + a, cy + b) around its word in as COLUMNS (vrc_word_columns.h): 40-bit values with the word at bit 4 and
// the two z layers beyond it below and above.  Rows and nibbles beyond the volume's faces are all `outside`.  27 loads, of which every neighbouring
// lane wants the same words: they are left to the caches.  The 26-count is separable, and every adder works on bit-planes,
// 32 voxels (40 with the nibbles) at a time:
//   x: per brick row, voxel x - 1, x and x + 1 at x's bit position (two shifts and the neighbour row's other half) go
//      through one full adder: 2 planes, 0 .. 3;
//   y: the planes of the rows cy - 1 and cy + 1 shifted to y's position, three 2-bit numbers added: 4 planes, 0 .. 9;
//   z: the 40-bit planes read at bit 0, 4 and 8 are the layers z - 1, z, z + 1 at the word's 32 positions, three 4-bit
//      numbers added: 5 planes, the count c27 of the 27 cells with the centre, 0 .. 27.
// The centre is folded into the rule, c26 = c27 - src: a solid centre looks c27 up in survive_mask << 1, an empty one in
// birth_mask.  A look-up is a select tree over the count planes, level by level, whose 32 leaves are the bits of the mask
// as all-ones or zero, the same for every lane; the centre selects between the two trees.  The 6-count is the direct sum
// of six planes (3 planes, 0 .. 6, an 8-leaf tree) from five rows.
// 4^3 has a branch of its own: a word holds the two brick rows cy = 0, 1 of one cx, 16 bits each with nibble k = z.  There
// a column is  outside | half | outside  and a lane runs the adders once per half (vrc_delta.hip: word_box and
// vrc_surface.hip: word_masks split that size off in the same way).
// `changed` is popc(dst ^ src) summed over the workgroup (vrc_group.h) into one 64-bit atomic; the kernel without a
// counter is an instantiation of its own.
//
// The fill.  One lane per destination word of the box's brick rows (vrc_box_words.h).  h(x, y, z) = L(L(L(L(seed) ^ x) ^ y) ^ z)
// nests in the order of a word's shape: L(seed) comes from the host, a word needs 2 values for its x, 4 for its (x, y) and
// then one L per voxel.  The word is stored under the box's mask by store_box_word, with the shared-word atomics of 4^3.
#include "vrc_cells.h"

#include "vrc_box_words.h"
#include "vrc_group.h"
#include "vrc_word_columns.h"

namespace {

template <class T>
__device__ __forceinline__ void full_add(T a, T b, T c, T& sum, T& carry)
{
    const T ab = a ^ b;
    sum = ab ^ c;
    carry = (a & b) | (ab & c);
}

// per voxel of a word, bit (table >> count) & 1 with count given as LEVELS bit-planes: a select tree whose leaves are the
// table's bits, uniform over the launch
template <int LEVELS>
__device__ __forceinline__ uint32_t look_up(uint32_t table, const uint32_t* planes)
{
    uint32_t v[1 << LEVELS];
#pragma unroll
    for (int i = 0; i < (1 << LEVELS); ++i) v[i] = 0u - ((table >> i) & 1u);
#pragma unroll
    for (int l = 0; l < LEVELS; ++l)
#pragma unroll
        for (int i = 0; i < (1 << (LEVELS - 1 - l)); ++i) v[i] = (planes[l] & v[2 * i + 1]) | (~planes[l] & v[2 * i]);
    return v[0];
}

// The new bits of the word wz of brick row (cx, cy) -- SMALL: of the half cy of word cx, in the low 16 bits -- and the
// word's (half's) source bits in *centre.
template <int NEIGH, bool SMALL>
__device__ __forceinline__ uint32_t rule(const WordColumns& f, int32_t cx, int32_t cy, uint32_t wz, uint32_t birth, uint32_t survive, uint32_t* centre)
{
    if (NEIGH == 6) {
        const uint64_t c = column<SMALL, true>(f, cx, cy, wz);
        const uint32_t xb = (uint32_t)(x_before(c, column<SMALL, false>(f, cx - 1, cy, wz)) >> 4);
        const uint32_t xa = (uint32_t)(x_after(c, column<SMALL, false>(f, cx + 1, cy, wz)) >> 4);
        const uint32_t yb = (uint32_t)(y_before(c, column<SMALL, false>(f, cx, cy - 1, wz)) >> 4);
        const uint32_t ya = (uint32_t)(y_after(c, column<SMALL, false>(f, cx, cy + 1, wz)) >> 4);
        const uint32_t zb = (uint32_t)c, za = (uint32_t)(c >> 8), own = (uint32_t)(c >> 4);
        uint32_t s, t, k, l, p[3];
        full_add(xb, xa, yb, s, k);                     // k, l: weight 2
        full_add(ya, zb, za, t, l);
        p[0] = s ^ t;
        full_add(k, l, s & t, p[1], p[2]);
        *centre = own;
        return (own & look_up<3>(survive, p)) | (~own & look_up<3>(birth, p));
    }
    // x: per brick row b = cy - 1, cy, cy + 1 the cells x - 1, x, x + 1 of every position, 0 .. 3 in two planes
    uint64_t s0[3], s1[3], own = 0ull;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const uint64_t c = column<SMALL, true>(f, cx, cy + b - 1, wz);
        full_add(x_before(c, column<SMALL, true>(f, cx - 1, cy + b - 1, wz)), c, x_after(c, column<SMALL, true>(f, cx + 1, cy + b - 1, wz)), s0[b], s1[b]);
        if (b == 1) own = c;
    }
    // y: three such numbers, 0 .. 9 in four planes t0 .. t3
    uint64_t t0, t1, t2, t3, k, u, v, w;
    full_add(y_before(s0[1], s0[0]), s0[1], y_after(s0[1], s0[2]), t0, k);             // k: weight 2
    full_add(y_before(s1[1], s1[0]), s1[1], y_after(s1[1], s1[2]), u, v);              // u: weight 2, v: weight 4
    t1 = u ^ k; w = u & k;                                                            // w: weight 4
    t2 = v ^ w; t3 = v & w;
    // z: the layers z - 1, z, z + 1 at the word's 32 positions, three numbers 0 .. 9, their sum 0 .. 27 in five planes
    const uint32_t d0 = (uint32_t)t0, d1 = (uint32_t)t1, d2 = (uint32_t)t2, d3 = (uint32_t)t3;
    const uint32_t c0 = (uint32_t)(t0 >> 4), c1 = (uint32_t)(t1 >> 4), c2 = (uint32_t)(t2 >> 4), c3 = (uint32_t)(t3 >> 4);
    const uint32_t u0 = (uint32_t)(t0 >> 8), u1 = (uint32_t)(t1 >> 8), u2 = (uint32_t)(t2 >> 8), u3 = (uint32_t)(t3 >> 8);
    uint32_t p[5], a, b2, b4a, b4b, b8a, b8b, b16a, b16b;
    full_add(d0, c0, u0, p[0], b2);
    full_add(d1, c1, u1, a, b4a);
    p[1] = a ^ b2; b4b = a & b2;
    full_add(d2, c2, u2, a, b8a);
    full_add(a, b4a, b4b, p[2], b8b);
    full_add(d3, c3, u3, a, b16a);
    full_add(a, b8a, b8b, p[3], b16b);
    p[4] = b16a | b16b;                                                               // the sum is below 32: never both
    const uint32_t o = (uint32_t)(own >> 4);
    *centre = o;
    // c26 = c27 - centre: a solid centre reads survive at c27 - 1
    return (o & look_up<5>(survive << 1, p)) | (~o & look_up<5>(birth, p));
}

// lg = log2 of the brick rows per axis.  A lane per word; the lanes beyond the field (8^3, 16^3 and 4^3 have fewer words
// than a workgroup has lanes) take part in the sum alone.
template <int NEIGH, bool COUNT>
__global__ __launch_bounds__(256) void k_cells_step(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t lg, uint32_t birth, uint32_t survive,
                                                    uint32_t edge, unsigned long long* __restrict__ changed)
{
    const uint32_t W = blockIdx.x * 256u + threadIdx.x;
    uint32_t flips = 0u;
    if (lg >= 2u) {
        // word (cx, cy, wz) of n / 4 words along z
        const uint32_t lgz = lg - 2u, n = 1u << lg;
        if (W < (1u << (2u * lg + lgz))) {
            const WordColumns f = {src, lg, edge};
            uint32_t centre;
            const uint32_t out = rule<NEIGH, false>(f, (int32_t)(W >> (lgz + lg)), (int32_t)((W >> lgz) & (n - 1u)), W & ((1u << lgz) - 1u), birth, survive, &centre);
            dst[W] = out;
            flips = (uint32_t)__popc(out ^ centre);
        }
    } else if (W < 2u) {
        // 4^3: word cx, its low half the brick row cy = 0 and its high half cy = 1
        const WordColumns f = {src, 1u, edge};
        uint32_t c0, c1;
        const uint32_t h0 = rule<NEIGH, true>(f, (int32_t)W, 0, 0u, birth, survive, &c0);
        const uint32_t h1 = rule<NEIGH, true>(f, (int32_t)W, 1, 0u, birth, survive, &c1);
        const uint32_t out = (h0 & 0xffffu) | (h1 << 16), centre = (c0 & 0xffffu) | (c1 << 16);
        dst[W] = out;
        flips = (uint32_t)__popc(out ^ centre);
    }
    if (COUNT) {
        __shared__ uint32_t part[4];
        const uint32_t all = group_sum<4u>(flips, part);                // at most 256 * 32
        if (threadIdx.x == 0 && all) atomicAdd(changed, (unsigned long long)all);
    }
}

// the 32-bit finaliser L of the fill's hash (include/vrc.h)
__host__ __device__ __forceinline__ uint32_t finalise(uint32_t u)
{
    u ^= u >> 16; u *= 0x7feb352du;
    u ^= u >> 15; u *= 0x846ca68bu;
    u ^= u >> 16;
    return u;
}

// seeded = L(seed).  A lane per word of the box's rows; the launch covers all items, no lane takes a second.
__global__ __launch_bounds__(256) void k_cells_fill_random(uint32_t* __restrict__ words, uint32_t S, uint32_t seeded, uint64_t threshold,
                                                           uint32_t lx, uint32_t ly, uint32_t lz, uint32_t hx, uint32_t hy, uint32_t hz, int op)
{
    const uint32_t lo[3] = {lx, ly, lz}, hi[3] = {hx, hy, hz};
    const uint32_t n = S >> 1;
    const BoxWords b = box_words(lo, hi);
    const uint64_t it = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (it >= b.items) return;
    RowWord r;
    if (!row_word(b, n, it, r)) return;
    const uint32_t mask = box_mask(b, r);
    if (!mask) return;
    uint32_t hxy[4];                                                    // k = yb * 2 + xb as in a brick's bit index
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) hxy[k] = finalise(finalise(seeded ^ (2u * r.cx + (k & 1u))) ^ (2u * r.cy + (k >> 1)));
    uint32_t bits = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        if (!((mask >> (8u * j)) & 0xffu)) continue;                    // also: a byte of another row (4^3)
        const uint32_t z0 = 2u * (uint32_t)(4u * r.w + j - r.base);
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i)
            if ((uint64_t)finalise(hxy[i & 3u] ^ (z0 + (i >> 2))) < threshold) bits |= 1u << (8u * j + i);
    }
    bits &= mask;
    store_box_word(words, r.w, mask, bits, op, n < 4u);
}

template <int NEIGH>
void launch_step(uint32_t* dst, const uint32_t* src, uint32_t depth, uint32_t birth, uint32_t survive, uint32_t edge, unsigned long long* changed, hipStream_t st)
{
    const uint32_t n_words = 1u << (3u * depth - 5u), groups = (n_words + 255u) / 256u;
    if (changed)
        hipLaunchKernelGGL((k_cells_step<NEIGH, true>), dim3(groups), dim3(256), 0, st, dst, src, depth - 1u, birth, survive, edge, changed);
    else
        hipLaunchKernelGGL((k_cells_step<NEIGH, false>), dim3(groups), dim3(256), 0, st, dst, src, depth - 1u, birth, survive, edge, changed);
}

}  // namespace

namespace vrc {

void cells_step_run(uint32_t* dst, const uint32_t* src, uint32_t depth, int neighbours, uint32_t birth_mask, uint32_t survive_mask, int outside,
                    unsigned long long* changed, hipStream_t st)
{
    const uint32_t edge = outside ? 0xffffffffu : 0u;
    if (neighbours == 6) launch_step<6>(dst, src, depth, birth_mask, survive_mask, edge, changed, st);
    else launch_step<26>(dst, src, depth, birth_mask, survive_mask, edge, changed, st);
}

void cells_fill_random_run(uint32_t* words, uint32_t depth, uint32_t seed, uint64_t threshold, const uint32_t lo[3], const uint32_t hi[3], int op,
                           hipStream_t st)
{
    const uint64_t groups = (box_word_items(lo, hi) + 255u) / 256u;      // at most 2^17 + 2^10: depth 10, the whole volume
    hipLaunchKernelGGL(k_cells_fill_random, dim3((uint32_t)groups), dim3(256), 0, st, words, 1u << depth, finalise(seed), threshold, lo[0], lo[1], lo[2],
                       hi[0], hi[1], hi[2], op);
}

}  // namespace vrc
