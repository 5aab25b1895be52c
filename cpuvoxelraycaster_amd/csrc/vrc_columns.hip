// vrc_columns.hip -- the occupancy along an axis (include/vrc.h: vrc_columns_profile, vrc_columns_fill, vrc_columns_select):
// what a column of voxels holds, a span per column from two height maps, and the voxels a parallel light reaches.
//
// The layout of a word (2 x 2 x 8 voxels, bit 4 k + 2 yb + xb with k = z & 7) is described at the top of vrc_flood.hip.  A
// LEVEL of a word is its voxels that share the coordinate along the axis, one bit per column that crosses the word:
//   x: 2 levels of 16 columns (yb, k), level j = (word >> j) & 0x55555555;
//   y: 2 levels of 16 columns (xb, k), level j = (word >> 2 j) & 0x33333333;
//   z: 8 levels of 4 columns (yb, xb), level j = (word >> 4 j) & 0xF.
// A BUNDLE is the columns that cross one word, and the walk of a bundle visits the words they cross in the order of the
// axis: along x the words (cx, cy, wz) for cx = 0 .. n - 1, a stride of a brick plane; along y a stride of a brick row; along z
// consecutive words.  Profile and select give every bundle to ONE lane, which walks it from face to face and carries the
// state of its 16 (4) columns as masks and bit-planes over the column positions of a level: no loop over voxels, no
// cross-lane step, and every word of the rect (of the volume) read once.  Lanes are numbered with wz fastest for x and y, so
// the strided walk loads 64 adjacent words per wave; along z a lane owns a brick row, adjacent lanes the next rows, and a
// row's words reach the lane one after another from the cache lines the first one brought in.  64-lane workgroups: at 512^3
// a walk along x or y has 16384 bundles, which 256-lane groups would put on 64 of the compute units.
//   profile: `seen` and `prev` masks, and four numbers per column in bit-planes: first and last as planes of the level's
//     coordinate (it is the same for every lane: a plane takes `fresh` or `solid` under a uniform all-ones / zero), count
//     and runs (solid & ~prev) by a ripple add of one bit.  The planes are read out column by column at the end and written
//     as 16-byte records, each once.  The walk always goes up the axis; the side only swaps first and last.
//   select: P - lo and P - hi as two's-complement numbers on 12 planes, initialised to -lo and -hi and raised by the level's
//     solid mask AFTER the level was judged: lo <= P < hi is ~sign(P - lo) & sign(P - hi).  The walk follows the direction.
//     The word goes out through store_selected_word.
// 4^3 has n = 2: a word holds the two brick rows cy = 0, 1 of one cx as halves of 16 bits.  The walk takes a half as a word
// whose levels 4 .. 7 along z are empty (shift and mask are part of the walk), and select stores the half with the
// shared-word atomics of store_box_word.
//
// fill: one lane per destination word of the box  rect x the whole axis  (vrc_box_words.h), written once through
// store_box_word under the box's mask.  Along z the lane reads the spans of its 4 columns and turns each into a mask of
// nibbles; along x and y it reads those of its 16 columns and compares the word's two levels.
#include "vrc_columns.h"

#include "vrc_box_words.h"
#include "vrc_fall.h"

namespace {

constexpr int COUNT_PLANES = 11;          // a count 0 .. 1024
constexpr int COORD_PLANES = 10;          // a coordinate 0 .. 1023, a number of runs 0 .. 512
constexpr int SIGNED_PLANES = 12;         // P - lo and P - hi, -1025 .. 1023
constexpr uint32_t WALK_GROUP = 64;       // lanes per workgroup of the two walks

template <int AXIS>
struct Shape {
    static constexpr int LEVELS = AXIS == 2 ? 8 : 2;                                   // of a word
    static constexpr int SHIFT = AXIS == 0 ? 1 : AXIS == 1 ? 2 : 4;                    // from a level to the next
    static constexpr uint32_t COLUMNS = AXIS == 0 ? 0x55555555u : AXIS == 1 ? 0x33333333u : 0xFu;
    static constexpr int N_COLUMNS = AXIS == 2 ? 4 : 16;
};

template <int AXIS>
__device__ __forceinline__ uint32_t level(uint32_t word, int j) { return (word >> (Shape<AXIS>::SHIFT * j)) & Shape<AXIS>::COLUMNS; }

// the bundles a rect touches, as a grid a0 .. a0 + na - 1 by b0 .. b0 + nb - 1: (cy, wz) for x, (cx, wz) for y, (cx, cy) for z
struct Bundles {
    uint32_t a0, na, b0, nb;
};

template <int AXIS>
__host__ __device__ __forceinline__ Bundles bundles(uint32_t u_lo, uint32_t v_lo, uint32_t u_hi, uint32_t v_hi)
{
    const uint32_t vs = AXIS == 2 ? 1u : 3u;
    return Bundles{u_lo >> 1, ((u_hi - 1u) >> 1) - (u_lo >> 1) + 1u, v_lo >> vs, ((v_hi - 1u) >> vs) - (v_lo >> vs) + 1u};
}

// column c of bundle (a, b): its bit in a level and its place (u, v) on the face
template <int AXIS>
__device__ __forceinline__ void column_of(int c, uint32_t a, uint32_t b, uint32_t* bit, uint32_t* u, uint32_t* v)
{
    const uint32_t hi = (uint32_t)c >> 1, lo = (uint32_t)c & 1u;
    if (AXIS == 0) { *bit = 4u * hi + 2u * lo; *u = 2u * a + lo; *v = 8u * b + hi; }         // (k, yb)
    else if (AXIS == 1) { *bit = 4u * hi + lo; *u = 2u * a + lo; *v = 8u * b + hi; }         // (k, xb)
    else { *bit = (uint32_t)c; *u = 2u * a + lo; *v = 2u * b + hi; }                         // (yb, xb)
}

// The walk of bundle (a, b) up the axis: word t is (words[idx + t idx_step] >> (shift + t shift_step)) & mask.
struct Walk {
    uint32_t idx;
    int32_t idx_step;
    uint32_t shift;
    int32_t shift_step;
    uint32_t mask, steps;
};

template <int AXIS>
__device__ __forceinline__ Walk walk_of(uint32_t lg, uint32_t a, uint32_t b)
{
    const uint32_t n = 1u << lg;
    if (lg < 2u) {
        // 4^3: word cx, half cy
        if (AXIS == 0) return Walk{0u, 1, 16u * a, 0, 0xffffu, 2u};
        if (AXIS == 1) return Walk{a, 0, 0u, 16, 0xffffu, 2u};
        return Walk{a, 0, 16u * b, 0, 0xffffu, 1u};
    }
    const uint32_t nwz = n >> 2;
    if (AXIS == 0) return Walk{a * nwz + b, (int32_t)(n * nwz), 0u, 0, 0xffffffffu, n};
    if (AXIS == 1) return Walk{a * n * nwz + b, (int32_t)nwz, 0u, 0, 0xffffffffu, n};
    return Walk{(a * n + b) * nwz, 1, 0u, 0, 0xffffffffu, nwz};
}

// planes += carry, one bit per column
template <int P>
__device__ __forceinline__ void add_bit(uint32_t (&planes)[P], uint32_t carry)
{
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const uint32_t t = planes[p] & carry;
        planes[p] ^= carry;
        carry = t;
    }
}

// the number the planes hold at column position `bit`
template <int P>
__device__ __forceinline__ uint32_t read_planes(const uint32_t (&planes)[P], uint32_t bit)
{
    uint32_t v = 0u;
#pragma unroll
    for (int p = 0; p < P; ++p) v |= ((planes[p] >> bit) & 1u) << p;
    return v;
}

// A lane per bundle of the rect; no lane takes a second one.
template <int AXIS>
__global__ __launch_bounds__(WALK_GROUP) void k_columns_profile(const uint32_t* __restrict__ words, uint32_t lg, int side, uint32_t u_lo, uint32_t v_lo,
                                                                uint32_t u_hi, uint32_t v_hi, vrc_column* __restrict__ out)
{
    constexpr int LEVELS = Shape<AXIS>::LEVELS;
    const Bundles g = bundles<AXIS>(u_lo, v_lo, u_hi, v_hi);
    const uint32_t it = blockIdx.x * WALK_GROUP + threadIdx.x;
    if (it >= g.na * g.nb) return;
    const uint32_t a = g.a0 + it / g.nb, b = g.b0 + it % g.nb;
    const Walk w = walk_of<AXIS>(lg, a, b);
    uint32_t seen = 0u, prev = 0u;
    uint32_t first[COORD_PLANES] = {}, last[COORD_PLANES] = {}, count[COUNT_PLANES] = {}, runs[COORD_PLANES] = {};
    uint32_t idx = w.idx, shift = w.shift;
#pragma unroll 2
    for (uint32_t t = 0; t < w.steps; ++t, idx += (uint32_t)w.idx_step, shift += (uint32_t)w.shift_step) {
        const uint32_t word = (words[idx] >> shift) & w.mask;
#pragma unroll
        for (int j = 0; j < LEVELS; ++j) {
            const uint32_t s = level<AXIS>(word, j), at = (uint32_t)LEVELS * t + (uint32_t)j;      // `at` is the same for every lane
            const uint32_t fresh = s & ~seen;
            seen |= s;
#pragma unroll
            for (int p = 0; p < COORD_PLANES; ++p) {
                const uint32_t one = 0u - ((at >> p) & 1u);
                first[p] |= fresh & one;
                last[p] = (last[p] & ~s) | (s & one);
            }
            add_bit(count, s);
            add_bit(runs, s & ~prev);
            prev = s;
        }
    }
    const uint32_t V = v_hi - v_lo;
#pragma unroll
    for (int c = 0; c < Shape<AXIS>::N_COLUMNS; ++c) {
        uint32_t bit, u, v;
        column_of<AXIS>(c, a, b, &bit, &u, &v);
        if (u < u_lo || u >= u_hi || v < v_lo || v >= v_hi) continue;          // also: the levels 4 .. 7 of a half of 4^3
        vrc_column r = {VRC_COLUMN_NONE, VRC_COLUMN_NONE, 0u, 0u};
        if ((seen >> bit) & 1u) {
            const uint32_t least = read_planes(first, bit), greatest = read_planes(last, bit);
            r.first = side ? least : greatest;
            r.last = side ? greatest : least;
            r.count = read_planes(count, bit);
            r.runs = read_planes(runs, bit);
        }
        out[(size_t)(u - u_lo) * V + (v - v_lo)] = r;
    }
}

// A lane per bundle of the volume, walking along the direction.  solid / empty: all ones where `of` selects them.
template <int AXIS>
__global__ __launch_bounds__(WALK_GROUP) void k_columns_select(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, uint32_t lg, int side, uint32_t lo,
                                                               uint32_t hi, uint32_t solid, uint32_t empty, int op)
{
    constexpr int LEVELS = Shape<AXIS>::LEVELS;
    const uint32_t S = 2u << lg;
    const Bundles g = bundles<AXIS>(0u, 0u, S, S);
    const uint32_t it = blockIdx.x * WALK_GROUP + threadIdx.x;
    if (it >= g.na * g.nb) return;
    const Walk w = walk_of<AXIS>(lg, it / g.nb, it % g.nb);
    uint32_t from_lo[SIGNED_PLANES], from_hi[SIGNED_PLANES];                   // P - lo and P - hi, P = 0
#pragma unroll
    for (int p = 0; p < SIGNED_PLANES; ++p) {
        from_lo[p] = 0u - (((0u - lo) >> p) & 1u);
        from_hi[p] = 0u - (((0u - hi) >> p) & 1u);
    }
    const uint32_t idx_step = side ? (uint32_t)w.idx_step : 0u - (uint32_t)w.idx_step;
    const uint32_t shift_step = side ? (uint32_t)w.shift_step : 0u - (uint32_t)w.shift_step;
    uint32_t idx = side ? w.idx : w.idx + (w.steps - 1u) * (uint32_t)w.idx_step;
    uint32_t shift = side ? w.shift : w.shift + (w.steps - 1u) * (uint32_t)w.shift_step;
#pragma unroll 2
    for (uint32_t t = 0; t < w.steps; ++t, idx += idx_step, shift += shift_step) {
        const uint32_t word = (src[idx] >> shift) & w.mask;
        uint32_t K = 0u;
#pragma unroll
        for (int i = 0; i < LEVELS; ++i) {
            const int j = side ? i : LEVELS - 1 - i;
            const uint32_t s = level<AXIS>(word, j);
            const uint32_t in_band = ~from_lo[SIGNED_PLANES - 1] & from_hi[SIGNED_PLANES - 1];
            K |= (in_band & ((s & solid) | (~s & empty)) & Shape<AXIS>::COLUMNS) << (Shape<AXIS>::SHIFT * j);
            add_bit(from_lo, s);
            add_bit(from_hi, s);
        }
        if (lg < 2u) store_box_word(dst, idx, w.mask << shift, (K & w.mask) << shift, op, true);
        else store_selected_word(dst, idx, K, op);
    }
}

// A lane per word of the box's rows; the launch covers all items, no lane takes a second.
template <int AXIS>
__global__ __launch_bounds__(256) void k_columns_fill(uint32_t* __restrict__ words, uint32_t S, uint32_t u_lo, uint32_t v_lo, uint32_t u_hi, uint32_t v_hi,
                                                      const int32_t* __restrict__ lo_map, int32_t lo_const, const int32_t* __restrict__ hi_map,
                                                      int32_t hi_const, int op)
{
    const uint32_t lo[3] = {AXIS == 0 ? 0u : u_lo, AXIS == 0 ? u_lo : AXIS == 1 ? 0u : v_lo, AXIS == 2 ? 0u : v_lo};
    const uint32_t hi[3] = {AXIS == 0 ? S : u_hi, AXIS == 0 ? u_hi : AXIS == 1 ? S : v_hi, AXIS == 2 ? S : v_hi};
    const uint32_t n = S >> 1, V = v_hi - v_lo;
    const BoxWords b = box_words(lo, hi);
    const uint64_t it = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (it >= b.items) return;
    RowWord r;
    if (!row_word(b, n, it, r)) return;
    const uint32_t mask = box_mask(b, r);
    if (!mask) return;
    // nibble q of the word is the row's level z = q + z_off (4^3: the half cy = 1 starts at nibble 4)
    const int32_t z_off = 2 * (int32_t)((int64_t)(4u * r.w) - (int64_t)r.base);
    uint32_t bits = 0u;
    if (AXIS == 2) {
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) {
            const uint32_t column = 0x11111111u << c;
            if (!(mask & column)) continue;
            const uint32_t e = (2u * r.cx + (c & 1u) - u_lo) * V + (2u * r.cy + (c >> 1) - v_lo);
            const int64_t from = (int64_t)(lo_map ? lo_map[e] : lo_const) - z_off, to = (int64_t)(hi_map ? hi_map[e] : hi_const) - z_off;
            const uint32_t q0 = (uint32_t)(from < 0 ? 0 : from > 8 ? 8 : from), q1 = (uint32_t)(to < 0 ? 0 : to > 8 ? 8 : to);
            if (q0 < q1) bits |= (uint32_t)(((1ull << (4u * q1)) - 1u) & ~((1ull << (4u * q0)) - 1u)) & column;
        }
    } else {
        const int32_t at = (int32_t)(2u * (AXIS == 0 ? r.cx : r.cy));       // the word's two levels: at, at + 1
#pragma unroll
        for (uint32_t c = 0; c < 16u; ++c) {
            const uint32_t q = c >> 1, other = c & 1u;
            const uint32_t bit0 = AXIS == 0 ? 4u * q + 2u * other : 4u * q + other, bit1 = bit0 + (AXIS == 0 ? 1u : 2u);
            if (!((mask >> bit0 | mask >> bit1) & 1u)) continue;
            const uint32_t e = (2u * (AXIS == 0 ? r.cy : r.cx) + other - u_lo) * V + ((uint32_t)((int32_t)q + z_off) - v_lo);
            const int32_t from = lo_map ? lo_map[e] : lo_const, to = hi_map ? hi_map[e] : hi_const;
            bits |= (uint32_t)(at >= from && at < to) << bit0 | (uint32_t)(at + 1 >= from && at + 1 < to) << bit1;
        }
    }
    store_box_word(words, r.w, mask, bits & mask, op, n < 4u);
}

template <int AXIS>
void launch_profile(const uint32_t* words, uint32_t depth, int side, const uint32_t rect[4], vrc_column* out, hipStream_t st)
{
    const Bundles g = bundles<AXIS>(rect[0], rect[1], rect[2], rect[3]);
    const uint32_t groups = (g.na * g.nb + WALK_GROUP - 1u) / WALK_GROUP;      // at most 2^18 bundles: z at 1024^3
    hipLaunchKernelGGL(k_columns_profile<AXIS>, dim3(groups), dim3(WALK_GROUP), 0, st, words, depth - 1u, side, rect[0], rect[1], rect[2], rect[3], out);
}

template <int AXIS>
void launch_select(uint32_t* dst, const uint32_t* src, uint32_t depth, int side, uint32_t lo, uint32_t hi, int of, int op, hipStream_t st)
{
    const uint32_t S = 1u << depth;
    const Bundles g = bundles<AXIS>(0u, 0u, S, S);
    const uint32_t groups = (g.na * g.nb + WALK_GROUP - 1u) / WALK_GROUP;
    hipLaunchKernelGGL(k_columns_select<AXIS>, dim3(groups), dim3(WALK_GROUP), 0, st, dst, src, depth - 1u, side, lo, hi,
                       (of & VRC_COLUMNS_SOLID) ? 0xffffffffu : 0u, (of & VRC_COLUMNS_EMPTY) ? 0xffffffffu : 0u, op);
}

template <int AXIS>
void launch_fill(uint32_t* words, uint32_t depth, const uint32_t rect[4], const int32_t* lo_map, int32_t lo_const, const int32_t* hi_map, int32_t hi_const,
                 int op, hipStream_t st)
{
    const uint32_t S = 1u << depth;
    const uint32_t lo[3] = {AXIS == 0 ? 0u : rect[0], AXIS == 0 ? rect[0] : AXIS == 1 ? 0u : rect[1], AXIS == 2 ? 0u : rect[1]};
    const uint32_t hi[3] = {AXIS == 0 ? S : rect[2], AXIS == 0 ? rect[2] : AXIS == 1 ? S : rect[3], AXIS == 2 ? S : rect[3]};
    const uint64_t groups = (box_word_items(lo, hi) + 255u) / 256u;            // at most 2^17 + 2^10: depth 10, the whole face
    hipLaunchKernelGGL(k_columns_fill<AXIS>, dim3((uint32_t)groups), dim3(256), 0, st, words, S, rect[0], rect[1], rect[2], rect[3], lo_map, lo_const,
                       hi_map, hi_const, op);
}

}  // namespace

namespace vrc {

void columns_profile_run(const uint32_t* words, uint32_t depth, int direction, const uint32_t rect[4], vrc_column* out, hipStream_t st)
{
    const int side = direction & 1;
    switch (fall_axis(direction)) {
    case 0: launch_profile<0>(words, depth, side, rect, out, st); break;
    case 1: launch_profile<1>(words, depth, side, rect, out, st); break;
    default: launch_profile<2>(words, depth, side, rect, out, st); break;
    }
}

void columns_fill_run(uint32_t* words, uint32_t depth, int axis, const uint32_t rect[4], const int32_t* lo_map, int32_t lo_const, const int32_t* hi_map,
                      int32_t hi_const, int op, hipStream_t st)
{
    switch (axis) {
    case 0: launch_fill<0>(words, depth, rect, lo_map, lo_const, hi_map, hi_const, op, st); break;
    case 1: launch_fill<1>(words, depth, rect, lo_map, lo_const, hi_map, hi_const, op, st); break;
    default: launch_fill<2>(words, depth, rect, lo_map, lo_const, hi_map, hi_const, op, st); break;
    }
}

void columns_select_run(uint32_t* dst, const uint32_t* src, uint32_t depth, int direction, uint32_t lo, uint32_t hi, int of, int op, hipStream_t st)
{
    const int side = direction & 1;
    switch (fall_axis(direction)) {
    case 0: launch_select<0>(dst, src, depth, side, lo, hi, of, op, st); break;
    case 1: launch_select<1>(dst, src, depth, side, lo, hi, of, op, st); break;
    default: launch_select<2>(dst, src, depth, side, lo, hi, of, op, st); break;
    }
}

}  // namespace vrc
