// vrc_stroke.h -- the capsule brush of the editable volume (include/vrc.h: vrc_stroke_*): which items are kept, how a capsule
// is cut into pieces along its major axis and the voxel box of each piece -- functions of values, no HIP call, so they run
// (and are tested, tests/test_stroke_host.py) on a machine without a device -- and the two launches as vrc_volume.hip calls
// them.  The kernels (vrc_stroke.hip) know occupancy words and item lists only; volumes, their ordering, the staging of host
// memory and k_hits_to_centres stay with vrc_volume.hip.
#pragma once
#include <stdint.h>

#include "../../include/vrc.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VRC_STROKE_HD __host__ __device__
#else
#define VRC_STROKE_HD
#endif

// voxels of the major axis to a piece: a multiple of 16, so that a piece starts on a word of the occupancy when z is the major
// axis and on a brick otherwise
#define VRC_STROKE_PIECE 16

namespace vrc {

struct Capsule {
    int32_t a[3], b[3], r;
};

// the rule for a dropped item (vrc.h): a coordinate or the radius beyond VRC_STROKE_LIMIT, or reserved != 0.  r < 0 is kept
// here and has no pieces.
VRC_STROKE_HD inline bool stroke_item_kept(const int32_t item[8])
{
    for (int i = 0; i < 6; ++i)
        if (item[i] > VRC_STROKE_LIMIT || item[i] < -VRC_STROKE_LIMIT) return false;
    return item[6] <= VRC_STROKE_LIMIT && item[7] == 0;
}

// The pieces of a kept capsule in a volume of S^3: slabs [first + k PIECE, first + (k + 1) PIECE) of the axis in which
// |b - a| is largest (the lowest such axis), cut to the capsule's own extent [lo, hi) on that axis, itself clipped to the
// volume.  count == 0: the capsule is empty (r < 0) or misses the volume on its major axis.
struct StrokePieces {
    int axis;
    int32_t lo, hi, first;
    uint32_t count;
};

VRC_STROKE_HD inline StrokePieces stroke_pieces(const Capsule& c, uint32_t S)
{
    StrokePieces ps;
    ps.axis = 0; ps.lo = ps.hi = ps.first = 0; ps.count = 0u;
    int32_t longest = -1;
    for (int j = 0; j < 3; ++j) {
        const int32_t d = c.b[j] - c.a[j], len = d < 0 ? -d : d;                 // <= 2^14
        if (len > longest) { longest = len; ps.axis = j; }
    }
    if (c.r < 0) return ps;
    const int32_t am = c.a[ps.axis], bm = c.b[ps.axis];
    const int32_t l = (am < bm ? am : bm) - c.r, h = (am < bm ? bm : am) + c.r + 1;   // |.| <= 2^14 + 1
    ps.lo = l < 0 ? 0 : l;
    ps.hi = h > (int32_t)S ? (int32_t)S : h;
    if (ps.lo >= ps.hi) return ps;
    ps.first = ps.lo & ~(VRC_STROKE_PIECE - 1);
    ps.count = (uint32_t)(ps.hi - ps.first + VRC_STROKE_PIECE - 1) / VRC_STROKE_PIECE;
    return ps;
}

// floor and ceiling of num / den for den > 0; |num| <= 2^28 here, and 32-bit divisions cost the device a fraction of 64-bit ones
VRC_STROKE_HD inline int32_t stroke_floor_div(int32_t num, int32_t den) { return num >= 0 ? num / den : -((-num + den - 1) / den); }
VRC_STROKE_HD inline int32_t stroke_ceil_div(int32_t num, int32_t den) { return -stroke_floor_div(-num, den); }

// The voxel box [lo, hi) of piece k < ps.count, clipped to the volume; false: it is empty.  A voxel p of the slab [m0, m1)
// that belongs to the capsule lies within r of its nearest point n of the segment, so n's major coordinate is in
// [m0 - r, m1 - 1 + r]: n is a point of the sub-segment between the major coordinates s and e below.  The segment is linear
// in its major coordinate, so on each other axis n lies between the sub-segment's two ends, and p within r of that: the box
// is those ends, rounded outward, grown by r.  The boxes of all pieces therefore hold every voxel of the capsule inside the
// volume; they may hold more, and the kernel tests every voxel against the whole capsule.
VRC_STROKE_HD inline bool stroke_piece_box(const Capsule& c, uint32_t S, const StrokePieces& ps, uint32_t k, uint32_t lo[3], uint32_t hi[3])
{
    const int M = ps.axis;
    const int32_t slab0 = ps.first + (int32_t)k * VRC_STROKE_PIECE, slab1 = slab0 + VRC_STROKE_PIECE;
    const int32_t m0 = slab0 < ps.lo ? ps.lo : slab0, m1 = slab1 > ps.hi ? ps.hi : slab1;
    if (m0 >= m1) return false;
    const int32_t am = c.a[M], bm = c.b[M];
    const int32_t mn = am < bm ? am : bm, mx = am < bm ? bm : am;
    const int32_t s = m0 - c.r > mn ? m0 - c.r : mn, e = m1 - 1 + c.r < mx ? m1 - 1 + c.r : mx;
    if (s > e) return false;                                                     // cannot be: [m0, m1) lies in [mn - r, mx + r]
    lo[M] = (uint32_t)m0; hi[M] = (uint32_t)m1;
    const int32_t dm = bm - am, den = dm < 0 ? -dm : dm;                         // <= 2^14
    for (int j = 0; j < 3; ++j) {
        if (j == M) continue;
        int32_t l = c.a[j], h = c.a[j];                                          // den == 0: a == b, the segment is a point
        if (den) {
            const int32_t dj = dm < 0 ? c.a[j] - c.b[j] : c.b[j] - c.a[j];       // |.| <= den
            const int32_t ns = (s - am) * dj, ne = (e - am) * dj;                // |s - am|, |e - am| <= den: |.| <= 2^28
            const int32_t fs = stroke_floor_div(ns, den), fe = stroke_floor_div(ne, den);   // |.| <= den
            const int32_t cs = stroke_ceil_div(ns, den), ce = stroke_ceil_div(ne, den);
            l = c.a[j] + (fs < fe ? fs : fe);
            h = c.a[j] + (cs > ce ? cs : ce);
        }
        l -= c.r; h += c.r + 1;                                                  // |.| < 2^15
        if (l < 0) l = 0;
        if (h > (int32_t)S) h = (int32_t)S;
        if (l >= h) return false;
        lo[j] = (uint32_t)l; hi[j] = (uint32_t)h;
    }
    return true;
}

#if defined(__HIPCC__)
// n capsules (n x 8 int32, vrc.h) into the occupancy words of a volume of `depth`: grid (n, split) of `lanes` threads.
void stroke_capsules_run(uint32_t* words, uint32_t depth, uint64_t n, const int32_t* items, uint32_t split, uint32_t lanes, int solid,
                         hipStream_t st);
// The stroke through n centres (n x 4 int32: x y z, radius or -1 for a record that is no centre, as k_hits_to_centres leaves
// them): item i is the capsule (c_i, c_i+1, radius) where both are centres and max_gap == 0 or |c_i+1 - c_i|^2 <= max_gap^2,
// the ball at c_i where only c_i is one, else nothing.  Read in place: no list of items is written.
void stroke_links_run(uint32_t* words, uint32_t depth, uint64_t n, const int32_t* centres, int32_t radius, uint32_t max_gap, uint32_t split,
                      uint32_t lanes, int solid, hipStream_t st);
#endif

}  // namespace vrc
