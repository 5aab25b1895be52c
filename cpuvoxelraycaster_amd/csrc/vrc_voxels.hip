// vrc_voxels.hip -- the solid voxels of the editable volume's bit field as a coordinate list, with the 27-bit
// neighbourhood of each where asked (include/vrc.h: vrc_voxels_count, vrc_voxels_extract): the inverse of
// vrc_volume_set_voxels.
//
// The layout of a word (2 x 2 x 8 voxels, bit zz*4 + yb*2 + xb) is described at the top of vrc_flood.hip.  A voxel's key
// is 32 W + bit, so the key order is (word, bit).  The three passes are vrc_list.h's with a lane = one word:
//   count: a lane's selection is  w & box mask & select(which)  -- for SURFACE / INTERIOR the union of the six face masks
//          of vrc_word_faces.h and its complement in w.  A lane whose word lies outside the box loads nothing, so a
//          workgroup wholly outside it writes 0 without touching the occupancy.  A slot is at most 256 * 32 = 8192;
//   emit:  every lane walks the set bits of its own mask.  x y z is one 8-byte and one 4-byte store, in the order the
//          record's address allows; x y z m is one 16-byte store.
// The neighbourhood.  A lane loads the 27 words around its word ONCE, as the nine brick rows (cx + a, cy + b) in the
// column form of vrc_word_columns.h.  Rows and nibbles beyond the volume are all `beyond`.  The x and y steps are the
// flood's shifts under WORD_X0 / X1 / Y0 / Y1, the z steps read the column at bit 0 / 4 / 8: 27 planes of 32 bits, plane
// k = 9 (dx + 1) + 3 (dy + 1) + (dz + 1) holding voxel c + (dx, dy, dz) at c's bit.  A voxel's m is bit b of each
// plane, and the six face planes (4, 22, 10, 16, 12, 14) give SURFACE / INTERIOR without the face masks.  4^3 (two
// words) takes every neighbour voxel by voxel from the rule, as the face masks do there.
// Word indices reach 2^25 and stay 32-bit; voxel indices reach 8^10 = 2^30 per list but are 64-bit throughout, as the
// window's bounds are.
#include "vrc_voxels.h"

#include "../../include/vrc.h"
#include "vrc_box_words.h"
#include "vrc_list.h"
#include "vrc_word_columns.h"
#include "vrc_word_faces.h"

namespace {

constexpr uint32_t GROUP = LIST_GROUP;        // words per workgroup

using vrc::VoxelQuery;

// the voxels of word W inside the box, as a mask of its bits; no load
__device__ __forceinline__ uint32_t word_box_mask(const Field& f, const VoxelQuery& q, uint32_t W)
{
    if (f.lg >= 2u) {
        const uint32_t lgz = f.lg - 2u, n = 1u << f.lg;
        const uint32_t wz = W & ((1u << lgz) - 1u), cy = (W >> lgz) & (n - 1u), cx = W >> (lgz + f.lg);
        const uint32_t xp = axis_pair(cx, q.lo[0], q.hi[0]), yp = axis_pair(cy, q.lo[1], q.hi[1]);
        const uint32_t layer = (((xp & 1u) ? 0x5u : 0u) | ((xp & 2u) ? 0xAu : 0u)) & (((yp & 1u) ? 0x3u : 0u) | ((yp & 2u) ? 0xCu : 0u));
        const uint32_t z0 = 8u * wz;
        const uint32_t zl = q.lo[2] > z0 ? q.lo[2] - z0 : 0u, zh = q.hi[2] < z0 + 8u ? (q.hi[2] > z0 ? q.hi[2] - z0 : 0u) : 8u;
        if (!layer || zl >= zh) return 0u;
        const uint32_t below_hi = zh == 8u ? 0xffffffffu : (1u << (4u * zh)) - 1u, below_lo = (1u << (4u * zl)) - 1u;
        return (layer * 0x11111111u) & below_hi & ~below_lo;
    }
    uint32_t mask = 0u;
    for (uint32_t bit = 0; bit < 32u; ++bit) {
        uint32_t c[3];
        voxel_of(f, W, bit, c);
        bool in = true;
        for (int a = 0; a < 3; ++a) in = in && c[a] >= q.lo[a] && c[a] < q.hi[a];
        if (in) mask |= 1u << bit;
    }
    return mask;
}

// the voxels of word W the list holds, from the word and its six face neighbours
__device__ __forceinline__ uint32_t selection(const Field& f, const VoxelQuery& q, uint32_t W)
{
    const uint32_t box = word_box_mask(f, q, W);
    if (!box) return 0u;
    if (q.which == VRC_VOXELS_ALL) return f.words[W] & box;
    uint32_t m[6];
    word_masks(f, W, m);
    const uint32_t exposed = m[0] | m[1] | m[2] | m[3] | m[4] | m[5];
    return (q.which == VRC_VOXELS_SURFACE ? exposed : f.words[W] & ~exposed) & box;
}

// the 27 planes of word W, lg >= 2: p[9 (dx+1) + 3 (dy+1) + (dz+1)] bit i = voxel (bit i of W) + (dx, dy, dz)
__device__ __forceinline__ void word_planes(const Field& f, uint32_t W, uint32_t p[27])
{
    const uint32_t lgz = f.lg - 2u, n = 1u << f.lg;
    const uint32_t wz = W & ((1u << lgz) - 1u);
    const int32_t cy = (int32_t)((W >> lgz) & (n - 1u)), cx = (int32_t)(W >> (lgz + f.lg));
    const WordColumns wc = {f.words, f.lg, f.beyond};
    uint64_t x[3][3];                          // [dx + 1][row cy + b - 1], at x's position
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const uint64_t c = column<false, true>(wc, cx, cy + b - 1, wz);
        x[0][b] = x_before(c, column<false, true>(wc, cx - 1, cy + b - 1, wz));
        x[1][b] = c;
        x[2][b] = x_after(c, column<false, true>(wc, cx + 1, cy + b - 1, wz));
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const uint64_t y[3] = {y_before(x[a][1], x[a][0]), x[a][1], y_after(x[a][1], x[a][2])};
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            p[9 * a + 3 * b + 0] = (uint32_t)y[b];
            p[9 * a + 3 * b + 1] = (uint32_t)(y[b] >> 4);
            p[9 * a + 3 * b + 2] = (uint32_t)(y[b] >> 8);
        }
    }
}

// the same selection from the planes, lg >= 2; the planes are loaded only where the word has a voxel in the box
__device__ __forceinline__ uint32_t selection_planes(const Field& f, const VoxelQuery& q, uint32_t W, uint32_t p[27])
{
    const uint32_t box = word_box_mask(f, q, W);
    if (!box) return 0u;
    const uint32_t w = f.words[W] & box;
    if (!w) return 0u;
    word_planes(f, W, p);
    const uint32_t enclosed = p[4] & p[22] & p[10] & p[16] & p[12] & p[14];
    return q.which == VRC_VOXELS_ALL ? w : q.which == VRC_VOXELS_SURFACE ? w & ~enclosed : w & enclosed;
}

// 4^3: the neighbourhood mask of voxel c from the rule itself
__device__ __forceinline__ uint32_t small_neighbourhood(const Field& f, const uint32_t c[3])
{
    const uint32_t both[2] = {f.words[0], f.words[1]};
    uint32_t m = 0u;
    for (int k = 0; k < 27; ++k) {
        const int32_t v[3] = {(int32_t)c[0] + k / 9 - 1, (int32_t)c[1] + (k / 3) % 3 - 1, (int32_t)c[2] + k % 3 - 1};
        m |= small_solid(both, f.beyond, v) << k;
    }
    return m;
}

__global__ __launch_bounds__(256) void k_voxels_count(Field f, VoxelQuery q, unsigned long long* __restrict__ slots)
{
    __shared__ uint32_t part[4];
    const uint32_t W = blockIdx.x * GROUP + threadIdx.x;
    const uint32_t sel = W < f.n_words ? selection(f, q, W) : 0u;
    const uint32_t s = group_sum<GROUP / 64u>(__popc(sel), part);
    if (threadIdx.x == 0) slots[blockIdx.x] = s;
}

// x y z at record `at` of a 4-byte aligned list: the 8-byte store goes where the record's address allows it
__device__ __forceinline__ void store_xyz(void* out, unsigned long long at, const uint32_t c[3])
{
    uint32_t* o = (uint32_t*)out + 3ull * at;
    if (((uintptr_t)o & 7u) == 0u) {
        *(uint2*)o = make_uint2(c[0], c[1]);
        o[2] = c[2];
    } else {
        o[0] = c[0];
        *(uint2*)(o + 1) = make_uint2(c[1], c[2]);
    }
}

template <int FORMAT>
__global__ __launch_bounds__(256) void k_voxels_emit(Field f, VoxelQuery q, const unsigned long long* __restrict__ slots, unsigned long long first,
                                                     unsigned long long capacity, void* out)
{
    __shared__ uint32_t part[GROUP / 64u];
    const uint32_t W = blockIdx.x * GROUP + threadIdx.x;
    const bool planes = FORMAT == VRC_VOXELS_NEIGHBOURS && f.lg >= 2u;   // uniform for the launch
    uint32_t p[27], sel = 0u;
    const auto count = [&]() {
        if (W < f.n_words) sel = planes ? selection_planes(f, q, W, p) : selection(f, q, W);
        return (uint32_t)__popc(sel);
    };
    unsigned long long idx, win_end;
    if (!list_window<GROUP / 64u>(slots, first, capacity, count, part, &idx, &win_end)) return;
    for (; sel; sel &= sel - 1u, ++idx) {
        if (idx < first || idx >= win_end) continue;
        const uint32_t bit = (uint32_t)__ffs((int)sel) - 1u;
        uint32_t c[3];
        voxel_of(f, W, bit, c);
        if (FORMAT == VRC_VOXELS_XYZ) {
            store_xyz(out, idx - first, c);
        } else {
            uint32_t m = 0u;
            if (planes) {
#pragma unroll
                for (int k = 0; k < 27; ++k) m |= ((p[k] >> bit) & 1u) << k;
            } else {
                m = small_neighbourhood(f, c);
            }
            ((uint4*)out)[idx - first] = make_uint4(c[0], c[1], c[2], m);
        }
    }
}

uint32_t groups_of(uint32_t depth) { return list_groups(1u << (3u * (depth - 1u) - 2u)); }

}  // namespace

namespace vrc {

size_t voxels_scratch_bytes(uint32_t depth) { return list_slot_bytes(groups_of(depth), false); }

unsigned long long* voxels_total_slot(unsigned long long* scratch, uint32_t depth) { return list_total_slot(scratch, groups_of(depth)); }

void voxels_offsets_run(const uint32_t* words, uint32_t depth, const VoxelQuery& q, unsigned long long* scratch, unsigned long long* d_total, hipStream_t st)
{
    hipLaunchKernelGGL(k_voxels_count, dim3(groups_of(depth)), dim3(GROUP), 0, st, field_of(words, depth, q.closed), q, scratch);
    // a slot <= 8192; a step's sum stays below 2^24
    hipLaunchKernelGGL(k_scan_slots<unsigned long long>, dim3(1), dim3(SCAN_GROUP), 0, st, scratch, groups_of(depth), d_total);
}

void voxels_emit_run(const uint32_t* words, uint32_t depth, const VoxelQuery& q, int format, uint64_t first, uint64_t capacity, void* out,
                     const unsigned long long* scratch, hipStream_t st)
{
    const Field f = field_of(words, depth, q.closed);
    const dim3 grid(groups_of(depth)), block(GROUP);
    const unsigned long long a = first, b = capacity;
    if (format == VRC_VOXELS_XYZ) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_voxels_emit<VRC_VOXELS_XYZ>), grid, block, 0, st, f, q, scratch, a, b, out);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_voxels_emit<VRC_VOXELS_NEIGHBOURS>), grid, block, 0, st, f, q, scratch, a, b, out);
}

}  // namespace vrc
