// vrc_rects.hip -- the exposed faces of the editable volume's bit field merged into rectangles, as a record or triangle
// list (include/vrc.h: vrc_rect_count, vrc_extract_rects).  It sits on top of vrc_surface.hip's face rule and
// count / scan / emit skeleton.
//
// The rule.  Direction d = 2 * axis + side has axis a; of the other two axes s < r, s is the stack axis and r the run axis.
// A row is the cells of one (d, c_a, c_s) indexed by c_r; a run [r0, r1) is a maximal set of consecutive exposed faces of a
// row; a rectangle is a maximal set of consecutive rows of one plane that hold the IDENTICAL run (maximal in each of them).
// A run starts a rectangle iff the row before does not hold it, and the rectangle's height is the number of rows after it
// that do.  Nothing depends on a sweep order, so every lane decides for itself.
//
// Rows as bits.  The brick words (2 x 2 x 8 voxels, bit (z & 7) * 4 + yb * 2 + xb: vrc_flood.hip) are first turned into two
// dense row fields of w = max(1, S / 32) words per row: Z-rows [x][y][z bits] for the axes x and y, Y-rows [x][z][y bits] for
// the axis z.  The faces of a row are then  row & ~(the same row of the plane c_a -/+ 1),  0 (closed) or ~0 (open) beyond the
// volume; bits past S of a row shorter than a word are 0.
//
// A pass over the rows, then the three passes of vrc_list.h, a lane = one word of one row in the canonical order
// (d, c_a, c_s, word) -- so a lane's rectangle starts in bit order continue the order (d, c_a, s0, r0):
//   rows:  one lane per word of the two fields gathers its 32 bits from the brick words;
//   count: the run starts of the word are m & ~(m << 1 | carry); a start whose row before starts no run there is a
//          rectangle start at once, the others follow their run to its end (across words) and test the row before for the
//          identical run.  A slot is at most 256 * 16;
//   emit:  a lane walks the rows after each of its starts inside the window to find the height, then writes one 16-byte
//          record, or nine 8-byte (or eighteen 4-byte) stores.
// Lane and word indices reach 6 * 2^25 and stay 32-bit; rectangle indices are 64-bit as the face indices are.
#include "vrc_rects.h"

#include "../../include/vrc.h"
#include "vrc_list.h"

namespace {

constexpr uint32_t GROUP = LIST_GROUP;        // lanes per workgroup

struct Rows {
    const uint32_t* zrows;                    // [x][y][z bits]
    const uint32_t* yrows;                    // [x][z][y bits]
    uint32_t depth;                           // S = 1 << depth
    uint32_t lgw;                             // log2 of the words per row
    uint32_t n_lanes;                         // 6 S^2 w
    uint32_t beyond;                          // what a row beyond the volume reads as: 0 closed, ~0 open
};

// ---- pass 0: the row fields --------------------------------------------------------------------------------------------

// bits 0, 4, .. 28 of t to bits 0 .. 7
__device__ __forceinline__ uint32_t every_fourth(uint32_t t)
{
    t &= 0x11111111u;
    t = (t | (t >> 3)) & 0x03030303u;
    t = (t | (t >> 6)) & 0x000f000fu;
    return (t | (t >> 12)) & 0xffu;
}

__global__ __launch_bounds__(256) void k_rect_rows(const uint32_t* __restrict__ words, uint32_t depth, uint32_t lgw, uint32_t* __restrict__ zrows,
                                                   uint32_t* __restrict__ yrows)
{
    const uint32_t S = 1u << depth, n_field = (S * S) << lgw;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= 2u * n_field) return;
    const bool along_y = i >= n_field;
    const uint32_t j = along_y ? i - n_field : i;
    const uint32_t k = j & ((1u << lgw) - 1u), q = (j >> lgw) & (S - 1u), p = j >> (lgw + depth);     // row (x = p, y or z = q)
    const uint32_t lg = depth - 1u;           // log2 of the bricks per axis
    uint32_t out = 0u;
    if (depth >= 5u) {
        const uint32_t lgz = lg - 2u;         // log2 of the words of a brick column along z
        if (!along_y) {
            // z = 32 k ..: four consecutive words of the brick column (x >> 1, y >> 1), eight z each
            const uint32_t W = (((((p >> 1) << lg) + (q >> 1)) << lgz) + 4u * k), sh = (q & 1u) * 2u + (p & 1u);
            const uint4 w = *(const uint4*)(words + W);
            out = every_fourth(w.x >> sh) | (every_fourth(w.y >> sh) << 8) | (every_fourth(w.z >> sh) << 16) | (every_fourth(w.w >> sh) << 24);
        } else {
            // y = 32 k ..: sixteen brick columns cy = 16 k .., two y each, of the word that holds z = q
            const uint32_t at = (q & 7u) * 4u + (p & 1u);
            for (uint32_t c = 0; c < 16u; ++c) {
                const uint32_t w = words[((((p >> 1) << lg) + 16u * k + c) << lgz) + (q >> 3)] >> at;
                out |= ((w & 1u) | ((w >> 1) & 2u)) << (2u * c);
            }
        }
    } else {
        // below 32^3 a row is shorter than a word (and at 4^3 an occupancy word straddles two brick rows): bit by bit
        for (uint32_t r = 0; r < S; ++r) {
            const uint32_t x = p, y = along_y ? r : q, z = along_y ? q : r;
            const uint32_t key = 8u * (((((x >> 1) << lg) + (y >> 1)) << lg) + (z >> 1)) + (z & 1u) * 4u + (y & 1u) * 2u + (x & 1u);
            out |= ((words[key >> 5] >> (key & 31u)) & 1u) << r;
        }
    }
    (along_y ? yrows : zrows)[j] = out;
}

// ---- the rule on the row fields ------------------------------------------------------------------------------------------

// the exposed faces of direction d in word k of row (c_a, c_s); all four inside the field
__device__ __forceinline__ uint32_t face_word(const Rows& f, uint32_t d, uint32_t ca, uint32_t cs, uint32_t k)
{
    const uint32_t a = d >> 1, S = 1u << f.depth;
    const uint32_t* __restrict__ field = a == 2u ? f.yrows : f.zrows;
    // x: row (x = c_a, y = c_s), the plane beside it S rows away; y and z: row (x = c_s, y or z = c_a), one row away
    const uint32_t row = a == 0u ? ca * S + cs : cs * S + ca, step = a == 0u ? S : 1u;
    const bool inside = (d & 1u) ? ca + 1u < S : ca > 0u;
    const uint32_t beside = inside ? ((d & 1u) ? row + step : row - step) : row;
    const uint32_t cur = field[(row << f.lgw) + k], nb = field[(beside << f.lgw) + k];
    return cur & ~(inside ? nb : f.beyond);
}

// where the run that covers bit b of word k (m = that word's faces) ends: r1
__device__ __forceinline__ uint32_t run_end(const Rows& f, uint32_t d, uint32_t ca, uint32_t cs, uint32_t k, uint32_t m, uint32_t b)
{
    uint32_t inv = ~m & (0xffffffffu << b);
    while (!inv) {
        if (++k == (1u << f.lgw)) return 32u * k;           // the row's end: only where S is a multiple of 32
        inv = ~face_word(f, d, ca, cs, k);
    }
    return 32u * k + (uint32_t)__ffs((int)inv) - 1u;
}

// does row cs (inside the field) hold [r0, r1) as a maximal run?
__device__ __forceinline__ bool holds_run(const Rows& f, uint32_t d, uint32_t ca, uint32_t cs, uint32_t r0, uint32_t r1)
{
    const uint32_t k0 = r0 >> 5, k1 = (r1 - 1u) >> 5;
    for (uint32_t k = k0; k <= k1; ++k) {
        const uint32_t w = face_word(f, d, ca, cs, k);
        const uint32_t lo = k == k0 ? r0 & 31u : 0u, hi = k == k1 ? (r1 - 1u) & 31u : 31u;     // inclusive
        const uint32_t mask = (0xffffffffu << lo) & (0xffffffffu >> (31u - hi));
        if ((w & mask) != mask) return false;
        if (lo && ((w >> (lo - 1u)) & 1u)) return false;
        if (hi < 31u && ((w >> (hi + 1u)) & 1u)) return false;
    }
    // the bits beside the run where they lie in another word
    if (!(r0 & 31u) && r0 && (face_word(f, d, ca, cs, k0 - 1u) >> 31)) return false;
    if (!(r1 & 31u) && r1 < (1u << f.depth) && (face_word(f, d, ca, cs, k1 + 1u) & 1u)) return false;
    return true;
}

struct Lane {
    uint32_t d, ca, cs, k;
    uint32_t m;                               // the faces of the lane's word
};

// the rectangle starts of lane L as a mask of its word's bits
__device__ __forceinline__ uint32_t rect_starts(const Rows& f, uint32_t L, Lane& at)
{
    const uint32_t S1 = (1u << f.depth) - 1u;
    at.k = L & ((1u << f.lgw) - 1u);
    uint32_t t = L >> f.lgw;
    at.cs = t & S1;
    t >>= f.depth;
    at.ca = t & S1;
    at.d = t >> f.depth;
    at.m = face_word(f, at.d, at.ca, at.cs, at.k);
    if (!at.m) return 0u;
    const uint32_t carry = at.k ? face_word(f, at.d, at.ca, at.cs, at.k - 1u) >> 31 : 0u;
    const uint32_t starts = at.m & ~((at.m << 1) | carry);
    if (!at.cs) return starts;
    // a run of the row before can only be identical where it starts at the same bit
    const uint32_t pm = face_word(f, at.d, at.ca, at.cs - 1u, at.k);
    const uint32_t pcarry = at.k ? face_word(f, at.d, at.ca, at.cs - 1u, at.k - 1u) >> 31 : 0u;
    uint32_t rs = starts & ~(pm & ~((pm << 1) | pcarry));
    for (uint32_t s = starts & ~rs; s; s &= s - 1u) {
        const uint32_t b = (uint32_t)__ffs((int)s) - 1u;
        if (!holds_run(f, at.d, at.ca, at.cs - 1u, 32u * at.k + b, run_end(f, at.d, at.ca, at.cs, at.k, at.m, b))) rs |= 1u << b;
    }
    return rs;
}

// DIRECTIONS: the six totals of the whole field (vrc_rect_count); otherwise the workgroup's own total
template <bool DIRECTIONS>
__global__ __launch_bounds__(256) void k_rect_count(Rows f, unsigned long long* __restrict__ slots)
{
    __shared__ uint32_t part[4];
    const uint32_t L = blockIdx.x * GROUP + threadIdx.x;
    Lane at;
    at.d = 6u;
    const uint32_t c = L < f.n_lanes ? __popc(rect_starts(f, L, at)) : 0u;
    if (DIRECTIONS) {
        // below 16^3 a workgroup spans several directions
        for (uint32_t d = 0; d < 6u; ++d) {
            const uint32_t s = group_sum<GROUP / 64u>(at.d == d ? c : 0u, part);
            if (threadIdx.x == 0 && s) atomicAdd(&slots[d], (unsigned long long)s);
        }
    } else {
        const uint32_t s = group_sum<GROUP / 64u>(c, part);
        if (threadIdx.x == 0) slots[blockIdx.x] = s;
    }
}

// WIDE: `out` is 8-byte aligned, a triangle pair goes out as nine 8-byte stores
template <int FORMAT, bool WIDE>
__global__ __launch_bounds__(256) void k_rect_emit(Rows f, const unsigned long long* __restrict__ slots, unsigned long long first,
                                                   unsigned long long capacity, void* out)
{
    __shared__ uint32_t part[GROUP / 64u];
    const uint32_t L = blockIdx.x * GROUP + threadIdx.x;
    Lane at;
    uint32_t rs = 0u;
    const auto count = [&]() {
        if (L < f.n_lanes) rs = rect_starts(f, L, at);
        return (uint32_t)__popc(rs);
    };
    unsigned long long idx, win_end;
    if (!list_window<GROUP / 64u>(slots, first, capacity, count, part, &idx, &win_end)) return;
    const uint32_t S = 1u << f.depth, a = at.d >> 1, side = at.d & 1u;
    for (; rs; rs &= rs - 1u, ++idx) {
        if (idx < first) continue;
        if (idx >= win_end) return;
        const uint32_t b = (uint32_t)__ffs((int)rs) - 1u;
        const uint32_t r0 = 32u * at.k + b, r1 = run_end(f, at.d, at.ca, at.cs, at.k, at.m, b);
        uint32_t ns = 1u;
        while (at.cs + ns < S && holds_run(f, at.d, at.ca, at.cs + ns, r0, r1)) ++ns;
        const uint32_t nr = r1 - r0;
        // x: s = y, r = z;  y: s = x, r = z;  z: s = x, r = y
        const uint32_t x = a == 0u ? at.ca : at.cs, y = a == 0u ? at.cs : a == 1u ? at.ca : r0, z = a == 2u ? at.ca : r0;
        const unsigned long long o = idx - first;
        if (FORMAT == VRC_SURFACE_FACES) {
            ((uint4*)out)[o] = make_uint4(x, y, z, at.d | ((nr - 1u) << 8) | ((ns - 1u) << 20));
            continue;
        }
        // the corner rule of include/vrc.h with the extents e: q0, q1 = q0 + U, q2 = q0 + U + V, q3 = q0 + V, where U lies
        // along u = (a + 1) % 3 and V along v = (a + 2) % 3
        const int32_t ex = a == 0u ? 1 : (int32_t)ns, ey = a == 0u ? (int32_t)ns : a == 1u ? 1 : (int32_t)nr, ez = a == 2u ? 1 : (int32_t)nr;
        const int32_t q0x = 64 * (int32_t)(x + (a == 0u ? side : 0u)), q0y = 64 * (int32_t)(y + (a == 1u ? side : 0u)),
                      q0z = 64 * (int32_t)(z + (a == 2u ? side : 0u));
        const int32_t ux = a == 2u ? 64 * ex : 0, uy = a == 0u ? 64 * ey : 0, uz = a == 1u ? 64 * ez : 0;
        const int32_t vx = a == 1u ? 64 * ex : 0, vy = a == 2u ? 64 * ey : 0, vz = a == 0u ? 64 * ez : 0;
        const int32_t q1x = q0x + ux, q1y = q0y + uy, q1z = q0z + uz;
        const int32_t q2x = q1x + vx, q2y = q1y + vy, q2z = q1z + vz;
        const int32_t q3x = q0x + vx, q3y = q0y + vy, q3z = q0z + vz;
        // side 1: (q0 q1 q2), (q0 q2 q3); side 0: (q0 q2 q1), (q0 q3 q2)
        const int32_t t[18] = {q0x, q0y, q0z, side ? q1x : q2x, side ? q1y : q2y, side ? q1z : q2z, side ? q2x : q1x, side ? q2y : q1y, side ? q2z : q1z,
                               q0x, q0y, q0z, side ? q2x : q3x, side ? q2y : q3y, side ? q2z : q3z, side ? q3x : q2x, side ? q3y : q2y, side ? q3z : q2z};
        store_triangle_pair<WIDE>(out, o, t);
    }
}

uint32_t words_lg(uint32_t depth) { return depth > 5u ? depth - 5u : 0u; }

uint32_t field_words(uint32_t depth) { return 1u << (2u * depth + words_lg(depth)); }

uint32_t lanes_of(uint32_t depth) { return 6u * field_words(depth); }

uint32_t groups_of(uint32_t depth) { return list_groups(lanes_of(depth)); }

// the two row fields lie behind the slots
uint32_t* fields_of(const unsigned long long* scratch, uint32_t depth) { return (uint32_t*)((const uint8_t*)scratch + list_slot_bytes(groups_of(depth), true)); }

Rows rows_of(const unsigned long long* scratch, uint32_t depth, int closed)
{
    Rows f;
    f.zrows = fields_of(scratch, depth);
    f.yrows = f.zrows + field_words(depth);
    f.depth = depth;
    f.lgw = words_lg(depth);
    f.n_lanes = lanes_of(depth);
    f.beyond = closed ? 0u : 0xffffffffu;
    return f;
}

}  // namespace

namespace vrc {

size_t rect_scratch_bytes(uint32_t depth) { return list_slot_bytes(groups_of(depth), true) + (size_t)field_words(depth) * 8u; }

unsigned long long* rect_total_slot(unsigned long long* scratch, uint32_t depth) { return list_total_slot(scratch, groups_of(depth)); }

unsigned long long* rect_direction_slots(unsigned long long* scratch, uint32_t depth) { return list_direction_slots(scratch, groups_of(depth)); }

void rect_rows_run(const uint32_t* words, uint32_t depth, unsigned long long* scratch, hipStream_t st)
{
    uint32_t* zrows = fields_of(scratch, depth);
    hipLaunchKernelGGL(k_rect_rows, dim3((2u * field_words(depth) + 255u) / 256u), dim3(256), 0, st, words, depth, words_lg(depth), zrows,
                       zrows + field_words(depth));
}

void rect_count_run(uint32_t depth, int closed, unsigned long long* scratch, hipStream_t st)
{
    unsigned long long* totals = rect_direction_slots(scratch, depth);
    (void)hipMemsetAsync(totals, 0, 48, st);
    hipLaunchKernelGGL(k_rect_count<true>, dim3(groups_of(depth)), dim3(GROUP), 0, st, rows_of(scratch, depth, closed), totals);
}

void rect_offsets_run(uint32_t depth, int closed, unsigned long long* scratch, unsigned long long* d_total, hipStream_t st)
{
    hipLaunchKernelGGL(k_rect_count<false>, dim3(groups_of(depth)), dim3(GROUP), 0, st, rows_of(scratch, depth, closed), scratch);
    // a slot <= 256 * 16; a step's sum stays below 2^22
    hipLaunchKernelGGL(k_scan_slots<unsigned long long>, dim3(1), dim3(SCAN_GROUP), 0, st, scratch, groups_of(depth), d_total);
}

void rect_emit_run(uint32_t depth, int closed, int format, uint64_t first, uint64_t capacity, void* out, const unsigned long long* scratch,
                   hipStream_t st)
{
    const auto kernel = emit_kernel_for(format, out, k_rect_emit<VRC_SURFACE_FACES, true>, k_rect_emit<VRC_SURFACE_TRIANGLES, true>,
                                        k_rect_emit<VRC_SURFACE_TRIANGLES, false>);
    hipLaunchKernelGGL(kernel, dim3(groups_of(depth)), dim3(GROUP), 0, st, rows_of(scratch, depth, closed), scratch, (unsigned long long)first,
                       (unsigned long long)capacity, out);
}

}  // namespace vrc
