// vrc_list.h -- what the windowed lists of the volume share (faces: vrc_surface.hip, voxels: vrc_voxels.hip, merged
// rectangles: vrc_rects.hip): the slot layout, the prologue of the emit pass, and the store of a triangle pair.
//
// A list is made in three passes on one stream.  A workgroup = LIST_GROUP consecutive lanes in the list's canonical order,
// a lane = one word of the field the list is read from; no workgroup waits for another:
//   1. count: every lane counts its records, the counts are summed over the workgroup (group_sum) into its slot;
//   2. scan:  one workgroup walks the slots SCAN_GROUP at a time and replaces them by their 64-bit exclusive prefix
//             (k_scan_slots); the total T goes behind the last slot;
//   3. emit:  a workgroup whose range [slot, next slot) misses the window [first, first + capacity) leaves after reading
//             the two slots.  The others recompute their counts, prefix them across their lanes, and every lane writes
//             those of its records that fall inside the window, at index - first.
// Passes 1 and 3 read the field once each; the writes of pass 3 follow the window.  Record indices are 64-bit throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vrc.h"
#include "vrc_group.h"

namespace {

constexpr uint32_t LIST_GROUP = 256;          // lanes per workgroup of the count and emit passes

// ---- the scratch block: a slot per workgroup, then the total, then (DIRECTIONS) six totals per face direction ------------

inline uint32_t list_groups(uint32_t lanes) { return (lanes + LIST_GROUP - 1u) / LIST_GROUP; }
inline size_t list_slot_bytes(uint32_t groups, bool directions) { return ((size_t)groups + (directions ? 7u : 1u)) * 8u; }
inline unsigned long long* list_total_slot(unsigned long long* scratch, uint32_t groups) { return scratch + groups; }
inline unsigned long long* list_direction_slots(unsigned long long* scratch, uint32_t groups) { return scratch + groups + 1u; }

// ---- pass 3 ----------------------------------------------------------------------------------------------------------------

// The prologue of an emit kernel, called by every lane of a workgroup of WAVES waves.  count() gives the lane's number of
// records (0 for a lane beyond the field); it runs only in a workgroup whose range meets the window.  true: this lane
// writes, its records start at list index *idx, and those with first <= index < *win_end go to index - first.
// The barrier rule: the first return is uniform for the workgroup and comes BEFORE the group scan, the second is per lane
// and comes AFTER it, so every lane of a workgroup that scans reaches both barriers of the scan.  No barrier may follow in
// the caller.  part: WAVES words of LDS.
template <uint32_t WAVES, class Count>
__device__ __forceinline__ bool list_window(const unsigned long long* __restrict__ slots, unsigned long long first, unsigned long long capacity,
                                            Count count, uint32_t* part, unsigned long long* idx, unsigned long long* win_end)
{
    const unsigned long long from = slots[blockIdx.x], to = slots[blockIdx.x + 1u];
    *win_end = capacity > ~0ull - first ? ~0ull : first + capacity;     // saturates: capacity may be the whole range
    if (from == to || to <= first || from >= *win_end) return false;
    const uint32_t mine = count();
    uint32_t all = 0u;
    *idx = from + group_exclusive_scan<WAVES>(mine, part, &all);
    return mine && *idx + mine > first && *idx < *win_end;
}

// the two triangles t (18 int32) to record `at` of a TRIANGLES list.  WIDE: `out` is 8-byte aligned, nine 8-byte stores
template <bool WIDE>
__device__ __forceinline__ void store_triangle_pair(void* out, unsigned long long at, const int32_t t[18])
{
    if (WIDE) {
        int2* o = (int2*)out + 9ull * at;
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = make_int2(t[2 * k], t[2 * k + 1]);
    } else {
        int32_t* o = (int32_t*)out + 18ull * at;
#pragma unroll
        for (int k = 0; k < 18; ++k) o[k] = t[k];
    }
}

// the emit kernel for a format and an output address, of a kernel template <FORMAT, WIDE> given as its three instances
template <class Kernel>
Kernel emit_kernel_for(int format, const void* out, Kernel faces, Kernel triangles_wide, Kernel triangles_narrow)
{
    if (format == VRC_SURFACE_FACES) return faces;
    return ((uintptr_t)out & 7u) == 0u ? triangles_wide : triangles_narrow;
}

}  // namespace
