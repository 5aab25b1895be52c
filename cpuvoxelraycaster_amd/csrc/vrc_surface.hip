// vrc_surface.hip -- the exposed faces of the editable volume's bit field as a face or triangle list (include/vrc.h:
// vrc_volume_surface_count, vrc_volume_extract_surface): the inverse of vrc_voxelize.hip.
//
// The exposed faces of a word in one direction are a mask of its bits, w & ~(the word's neighbours shifted onto it):
// word_masks in vrc_word_faces.h, which the voxel lists (vrc_voxels.hip) share.  No voxel is expanded to a byte.
//
// The canonical order is (word, direction, bit), the three passes are vrc_list.h's with a lane = one word: a lane counts
// the popcounts of its six masks (a slot is at most 256 * 192 faces), and in the emit pass walks the set bits of its own
// word: one 16-byte store per face record, nine 8-byte (or eighteen 4-byte) stores per pair of triangles.
// Each pass reads every word and its six neighbours once (the neighbours come from the caches: a word is the x / y / z
// neighbour of six others).  Word indices reach 2^25 and stay 32-bit, face indices reach 3 * 8^10 > 2^32.
#include "vrc_surface.h"

#include "../../include/vrc.h"
#include "vrc_list.h"
#include "vrc_word_faces.h"

namespace {

constexpr uint32_t GROUP = LIST_GROUP;        // words per workgroup

// DIRECTIONS: the six totals of the whole field (vrc_volume_surface_count); otherwise the workgroup's own total
template <bool DIRECTIONS>
__global__ __launch_bounds__(256) void k_surface_count(Field f, unsigned long long* __restrict__ slots)
{
    __shared__ uint32_t part[4];
    const uint32_t W = blockIdx.x * GROUP + threadIdx.x;
    uint32_t m[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (W < f.n_words) word_masks(f, W, m);
    if (DIRECTIONS) {
        for (int d = 0; d < 6; ++d) {
            const uint32_t s = group_sum<GROUP / 64u>(__popc(m[d]), part);
            if (threadIdx.x == 0 && s) atomicAdd(&slots[d], (unsigned long long)s);
        }
    } else {
        uint32_t c = 0u;
        for (int d = 0; d < 6; ++d) c += __popc(m[d]);
        const uint32_t s = group_sum<GROUP / 64u>(c, part);
        if (threadIdx.x == 0) slots[blockIdx.x] = s;
    }
}

// the two triangles of face d of voxel c, 18 int32 in vrc_volume_xor_mesh's units (include/vrc.h: the corner rule)
template <int D>
__device__ __forceinline__ void face_triangles(const uint32_t c[3], int32_t t[18])
{
    constexpr int a = D >> 1, side = D & 1, u = (a + 1) % 3, v = (a + 2) % 3;
    const int32_t pa = 64 * (int32_t)(c[a] + (uint32_t)side), u0 = 64 * (int32_t)c[u], v0 = 64 * (int32_t)c[v], u1 = u0 + 64, v1 = v0 + 64;
    int32_t q[4][3];
    q[0][a] = pa; q[0][u] = u0; q[0][v] = v0;
    q[1][a] = pa; q[1][u] = u1; q[1][v] = v0;
    q[2][a] = pa; q[2][u] = u1; q[2][v] = v1;
    q[3][a] = pa; q[3][u] = u0; q[3][v] = v1;
    constexpr int order[2][6] = {{0, 2, 1, 0, 3, 2}, {0, 1, 2, 0, 2, 3}};
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) t[3 * k + j] = q[order[side][k]][j];
}

// the faces of direction D of one word, from face index idx on; returns the index behind them
template <int FORMAT, bool WIDE, int D>
__device__ __forceinline__ unsigned long long emit_direction(const Field& f, uint32_t W, uint32_t m, unsigned long long idx, unsigned long long first,
                                                             unsigned long long win_end, void* out)
{
    const unsigned long long end = idx + __popc(m);
    if (end <= first || idx >= win_end) return end;
    while (m) {
        const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        if (idx >= first && idx < win_end) {
            uint32_t c[3];
            voxel_of(f, W, bit, c);
            const unsigned long long at = idx - first;
            if (FORMAT == VRC_SURFACE_FACES) {
                ((uint4*)out)[at] = make_uint4(c[0], c[1], c[2], (uint32_t)D);
            } else {
                int32_t t[18];
                face_triangles<D>(c, t);
                store_triangle_pair<WIDE>(out, at, t);
            }
        }
        ++idx;
    }
    return end;
}

// WIDE: `out` is 8-byte aligned, a triangle pair goes out as nine 8-byte stores
template <int FORMAT, bool WIDE>
__global__ __launch_bounds__(256) void k_surface_emit(Field f, const unsigned long long* __restrict__ slots, unsigned long long first,
                                                      unsigned long long capacity, void* out)
{
    __shared__ uint32_t part[GROUP / 64u];
    const uint32_t W = blockIdx.x * GROUP + threadIdx.x;
    uint32_t m[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    const auto count = [&]() {
        if (W < f.n_words) word_masks(f, W, m);
        uint32_t mine = 0u;
        for (int d = 0; d < 6; ++d) mine += __popc(m[d]);
        return mine;
    };
    unsigned long long idx, win_end;
    if (!list_window<GROUP / 64u>(slots, first, capacity, count, part, &idx, &win_end)) return;
    idx = emit_direction<FORMAT, WIDE, 0>(f, W, m[0], idx, first, win_end, out);
    idx = emit_direction<FORMAT, WIDE, 1>(f, W, m[1], idx, first, win_end, out);
    idx = emit_direction<FORMAT, WIDE, 2>(f, W, m[2], idx, first, win_end, out);
    idx = emit_direction<FORMAT, WIDE, 3>(f, W, m[3], idx, first, win_end, out);
    idx = emit_direction<FORMAT, WIDE, 4>(f, W, m[4], idx, first, win_end, out);
    emit_direction<FORMAT, WIDE, 5>(f, W, m[5], idx, first, win_end, out);
}

uint32_t groups_of(uint32_t depth) { return list_groups(1u << (3u * (depth - 1u) - 2u)); }

}  // namespace

namespace vrc {

size_t surface_scratch_bytes(uint32_t depth) { return list_slot_bytes(groups_of(depth), true); }

unsigned long long* surface_total_slot(unsigned long long* scratch, uint32_t depth) { return list_total_slot(scratch, groups_of(depth)); }

unsigned long long* surface_direction_slots(unsigned long long* scratch, uint32_t depth) { return list_direction_slots(scratch, groups_of(depth)); }

void surface_count_run(const uint32_t* words, uint32_t depth, int closed, unsigned long long* scratch, hipStream_t st)
{
    unsigned long long* totals = surface_direction_slots(scratch, depth);
    (void)hipMemsetAsync(totals, 0, 48, st);
    hipLaunchKernelGGL(k_surface_count<true>, dim3(groups_of(depth)), dim3(GROUP), 0, st, field_of(words, depth, closed), totals);
}

void surface_offsets_run(const uint32_t* words, uint32_t depth, int closed, unsigned long long* scratch, unsigned long long* d_total, hipStream_t st)
{
    hipLaunchKernelGGL(k_surface_count<false>, dim3(groups_of(depth)), dim3(GROUP), 0, st, field_of(words, depth, closed), scratch);
    // a slot <= 256 * 192; a step's sum stays below 2^26
    hipLaunchKernelGGL(k_scan_slots<unsigned long long>, dim3(1), dim3(SCAN_GROUP), 0, st, scratch, groups_of(depth), d_total);
}

void surface_emit_run(const uint32_t* words, uint32_t depth, int closed, int format, uint64_t first, uint64_t capacity, void* out,
                      const unsigned long long* scratch, hipStream_t st)
{
    const auto kernel = emit_kernel_for(format, out, k_surface_emit<VRC_SURFACE_FACES, true>, k_surface_emit<VRC_SURFACE_TRIANGLES, true>,
                                        k_surface_emit<VRC_SURFACE_TRIANGLES, false>);
    hipLaunchKernelGGL(kernel, dim3(groups_of(depth)), dim3(GROUP), 0, st, field_of(words, depth, closed), scratch, (unsigned long long)first,
                       (unsigned long long)capacity, out);
}

}  // namespace vrc
