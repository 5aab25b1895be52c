// vrc_raster.h -- surface voxelisation of triangle meshes (include/vrc.h: vrc_raster_mesh; the surface half of Schwarz &
// Seidel, "Fast parallel surface and solid voxelization on GPUs", 2010, of which vrc_voxelize.hip is the solid half): the two
// rules as functions of values -- no HIP type, so the same text runs on the device and on a machine without one
// (tests/cpp/raster_rule_main.cpp holds the pruning to the predicate by brute force) -- and the launch as vrc_volume.hip calls it.
//
// Units are vrc_volume_xor_mesh's: 64 per voxel, voxel p is the closed cube [64p, 64p + 64]^3 with its centre at 64p + 32.  All
// arithmetic is int64; with |coordinate| <= 2^17 an edge is below 2^18, a normal component below 2^37 and every dot product
// below 2^57.
//
// TOUCHED is decided by raster_touches: the 13 separating axes (raster_axis), non-strict.  What the kernel visits is pruned by
// raster_plan / raster_item, which apply some of those axes in closed form and therefore never drop a voxel the predicate accepts:
//   * a triangle with n != 0 is walked by the voxel columns of its projection along the dominant axis a (the lowest axis with
//     the largest |n_a|).  A column leaves on the three edge axes e_a x (Q - P), which do not depend on p_a; the plane axis and
//     the unit axis a then give a closed interval of p_a, at most (|n_u| + |n_v| + |n_a|) / |n_a| + 2 <= 5 voxels long.
//   * a triangle with n == 0 is a segment (or a point): it is walked by the slabs of its longest axis, and a slab's piece of the
//     segment, rounded outward, touches at most 3 x 3 columns.
// Cost, one triangle corner to corner of 512^3, (0,0,0) (S,S,0) (S,0,S) in voxels (tests/cpp/raster_rule_main.cpp prints the
// three figures): the predicate is applied to 524 287 voxels and selects every one of them -- all three components of n are
// equal in size there, and each column's interval is its four voxels -- where the bounding box holds 134 217 728, 256 times as many.
//
// Time at 512^3 on the MI355X (tools/bench_raster.py, profiles/edit/raster_timing.json; device time, set + clear, median of 5):
// the terrain's 583 244 merged-rectangle triangles TOUCHED 37.6 ms, THIN 2.02 ms, vrc_volume_xor_mesh twice 1.02 ms; the
// corner-to-corner triangle TOUCHED 0.272 ms, THIN 0.044 ms, vrc_volume_fill_boxes of its bounding box 0.052 ms; 100 000 unit-face
// triangles TOUCHED 5.46 ms, THIN 0.49 ms, xor_mesh twice 0.184 ms.  TOUCHED is 5 to 37 times slower than its yardsticks and costs
// about 30 ns per triangle of a large batch whatever the triangle's size: per workgroup, not per voxel.
//
// THIN's cover test (raster_covered) is vrc_volume_xor_mesh's Cover rule with (x, y, z) replaced by (u, v, a).  It is a second
// copy of the dozen lines of k_mark_triangles and not shared with them: that kernel's text stays as it is.
#pragma once
#include <stdint.h>

#include "../../include/vrc.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VRC_RASTER_HD __host__ __device__
#else
#define VRC_RASTER_HD
#endif

#define VRC_RASTER_LIMIT (1 << 17)             // |coordinate| in 1/64 voxel, as vrc_volume_xor_mesh

namespace vrc {

// a triangle with a coordinate beyond the limit is dropped; v = its coordinates widened
VRC_RASTER_HD inline bool raster_tri_kept(const int32_t t[9], int64_t v[9])
{
    for (int i = 0; i < 9; ++i) {
        if (t[i] > VRC_RASTER_LIMIT || t[i] < -VRC_RASTER_LIMIT) return false;
        v[i] = t[i];
    }
    return true;
}

// floor and ceiling of num / den for den > 0
VRC_RASTER_HD inline int64_t raster_floor_div(int64_t num, int64_t den)
{
    const int64_t q = num / den;
    return (num % den != 0 && num < 0) ? q - 1 : q;
}
VRC_RASTER_HD inline int64_t raster_ceil_div(int64_t num, int64_t den) { return -raster_floor_div(-num, den); }

VRC_RASTER_HD inline void raster_normal(const int64_t v[9], int64_t n[3])
{
    const int64_t ux = v[3] - v[0], uy = v[4] - v[1], uz = v[5] - v[2], wx = v[6] - v[0], wy = v[7] - v[1], wz = v[8] - v[2];
    n[0] = uy * wz - uz * wy; n[1] = uz * wx - ux * wz; n[2] = ux * wy - uy * wx;
}

// ---- TOUCHED: the predicate ----------------------------------------------------------------------------------------------------

// One separating axis L, with the triangle's and the cube's extents folded into two bounds: the intervals of vrc.h overlap iff
// lo <= L.o <= hi for o = 64p (lo = min L.V - 64 sum max(L_i, 0), hi = max L.V - 64 sum min(L_i, 0)).  L == 0 gives 0 <= 0 <= 0.
struct RasterAxis {
    int64_t L[3], lo, hi;
};

// axis k of the 13: 0..2 the unit axes, 3 the normal, 4 + 3e + a = e_a x (Q - P) for edge e (A->B, B->C, C->A)
VRC_RASTER_HD inline RasterAxis raster_axis(const int64_t v[9], int k)
{
    RasterAxis x;
    x.L[0] = x.L[1] = x.L[2] = 0;
    if (k < 3) x.L[k] = 1;
    else if (k == 3) raster_normal(v, x.L);
    else {
        const int e = (k - 4) / 3, a = (k - 4) % 3, u = (a + 1) % 3, w = (a + 2) % 3;
        const int64_t* P = v + 3 * e;
        const int64_t* Q = v + 3 * ((e + 1) % 3);
        x.L[u] = -(Q[w] - P[w]);                                        // e_a x d = (0, -d_w, d_u) in (a, u, w)
        x.L[w] = Q[u] - P[u];
    }
    int64_t mn = 0, mx = 0, neg = 0, pos = 0;
    for (int j = 0; j < 3; ++j) {
        const int64_t d = x.L[0] * v[3 * j] + x.L[1] * v[3 * j + 1] + x.L[2] * v[3 * j + 2];
        if (j == 0 || d < mn) mn = d;
        if (j == 0 || d > mx) mx = d;
        if (x.L[j] < 0) neg += x.L[j]; else pos += x.L[j];
    }
    x.lo = mn - 64 * pos;
    x.hi = mx - 64 * neg;
    return x;
}

VRC_RASTER_HD inline bool raster_axis_ok(const RasterAxis& x, const int64_t p[3])
{
    const int64_t d = 64 * (x.L[0] * p[0] + x.L[1] * p[1] + x.L[2] * p[2]);
    return x.lo <= d && d <= x.hi;
}

// the predicate: voxel p's closed cube and the closed triangle share a point
VRC_RASTER_HD inline bool raster_touches(const RasterAxis axes[13], const int64_t p[3])
{
    for (int k = 0; k < 13; ++k)
        if (!raster_axis_ok(axes[k], p)) return false;
    return true;
}

// ---- TOUCHED: what is visited --------------------------------------------------------------------------------------------------

struct RasterPlan {
    int kind;                  // 0: nothing to visit; 1: a triangle by columns; 2: a segment by slabs
    int a, u, w;               // the dominant (kind 1) or longest (kind 2) axis and the two others, (a + 1) % 3 and (a + 2) % 3
    int64_t lo[3], hi[3];      // the voxels whose cube meets the triangle's bounding box, clipped to the volume; inclusive
    uint32_t items;            // kind 1: columns (u, w) of that box; kind 2: its slabs along a
    // kind 1: the normal with n[a] > 0, n.A, and 64 times the sums of its negative and positive components
    int64_t n[3], nA, neg64, pos64;
    // kind 2: the segment's ends, P[a] <= Q[a]
    int64_t P[3], Q[3];
};

VRC_RASTER_HD inline RasterPlan raster_plan(const int64_t v[9], uint32_t S)
{
    RasterPlan pl;
    pl.kind = 0; pl.a = 0; pl.u = 1; pl.w = 2; pl.items = 0u;
    pl.nA = pl.neg64 = pl.pos64 = 0;
    int64_t extent[3];
    bool empty = false;
    for (int j = 0; j < 3; ++j) {
        int64_t mn = v[j], mx = v[j];
        for (int k = 1; k < 3; ++k) {
            mn = v[3 * k + j] < mn ? v[3 * k + j] : mn;
            mx = v[3 * k + j] > mx ? v[3 * k + j] : mx;
        }
        extent[j] = mx - mn;
        pl.lo[j] = (mn - 1) >> 6;                                       // ceil((mn - 64) / 64)
        pl.hi[j] = mx >> 6;                                             // floor(mx / 64)
        if (pl.lo[j] < 0) pl.lo[j] = 0;
        if (pl.hi[j] > (int64_t)S - 1) pl.hi[j] = (int64_t)S - 1;
        if (pl.lo[j] > pl.hi[j]) empty = true;
        pl.n[j] = 0; pl.P[j] = pl.Q[j] = v[j];
    }
    if (empty) return pl;
    int64_t n[3];
    raster_normal(v, n);
    if (n[0] != 0 || n[1] != 0 || n[2] != 0) {
        int64_t best = -1;
        for (int j = 0; j < 3; ++j) {
            const int64_t m = n[j] < 0 ? -n[j] : n[j];
            if (m > best) { best = m; pl.a = j; }
        }
        pl.kind = 1;
        pl.u = (pl.a + 1) % 3; pl.w = (pl.a + 2) % 3;
        const int64_t s = n[pl.a] > 0 ? 1 : -1;
        for (int j = 0; j < 3; ++j) {
            pl.n[j] = s * n[j];
            pl.nA += pl.n[j] * v[j];
            if (pl.n[j] < 0) pl.neg64 += 64 * pl.n[j]; else pl.pos64 += 64 * pl.n[j];
        }
        pl.items = (uint32_t)((pl.hi[pl.u] - pl.lo[pl.u] + 1) * (pl.hi[pl.w] - pl.lo[pl.w] + 1));    // at most 2^20
        return pl;
    }
    int64_t longest = -1;
    for (int j = 0; j < 3; ++j)
        if (extent[j] > longest) { longest = extent[j]; pl.a = j; }
    pl.kind = 2;
    pl.u = (pl.a + 1) % 3; pl.w = (pl.a + 2) % 3;
    for (int k = 1; k < 3; ++k) {
        if (v[3 * k + pl.a] < pl.P[pl.a])
            for (int j = 0; j < 3; ++j) pl.P[j] = v[3 * k + j];
        if (v[3 * k + pl.a] > pl.Q[pl.a])
            for (int j = 0; j < 3; ++j) pl.Q[j] = v[3 * k + j];
    }
    pl.items = (uint32_t)(pl.hi[pl.a] - pl.lo[pl.a] + 1);
    return pl;
}

// The voxels to which the predicate is applied for item < pl.items: the box [lo, hi], inclusive, inside pl's own; false: none.
VRC_RASTER_HD inline bool raster_item(const RasterPlan& pl, const RasterAxis axes[13], uint32_t item, int64_t lo[3], int64_t hi[3])
{
    const int a = pl.a, u = pl.u, w = pl.w;
    if (pl.kind == 1) {
        const uint32_t nw = (uint32_t)(pl.hi[w] - pl.lo[w] + 1);
        int64_t p[3];
        p[u] = pl.lo[u] + item / nw; p[w] = pl.lo[w] + item % nw; p[a] = 0;
        for (int e = 0; e < 3; ++e)
            if (!raster_axis_ok(axes[4 + 3 * e + a], p)) return false;  // L[a] == 0: whatever p[a]
        // the plane: n.o + neg64 <= n.A <= n.o + pos64 with o = 64p, solved for p[a]
        const int64_t K = pl.nA - 64 * (pl.n[u] * p[u] + pl.n[w] * p[w]), D = 64 * pl.n[a];
        int64_t l = raster_ceil_div(K - pl.pos64, D), h = raster_floor_div(K - pl.neg64, D);
        if (l < pl.lo[a]) l = pl.lo[a];
        if (h > pl.hi[a]) h = pl.hi[a];
        if (l > h) return false;
        lo[u] = hi[u] = p[u]; lo[w] = hi[w] = p[w];
        lo[a] = l; hi[a] = h;
        return true;
    }
    if (pl.kind != 2) return false;
    // the slab's piece of the segment: a in [m0, m1], the other coordinates between their values at the two ends, rounded outward
    const int64_t slab = pl.lo[a] + item;
    const int64_t m0 = 64 * slab > pl.P[a] ? 64 * slab : pl.P[a], m1 = 64 * slab + 64 < pl.Q[a] ? 64 * slab + 64 : pl.Q[a];
    if (m0 > m1) return false;                                          // cannot be: the slab meets [P[a], Q[a]]
    lo[a] = hi[a] = slab;
    const int64_t den = pl.Q[a] - pl.P[a];
    const int others[2] = {u, w};
    for (int i = 0; i < 2; ++i) {
        const int j = others[i];
        int64_t l = pl.P[j], h = pl.P[j];                               // den == 0: a point
        if (den) {
            const int64_t dj = pl.Q[j] - pl.P[j], n0 = (m0 - pl.P[a]) * dj, n1 = (m1 - pl.P[a]) * dj;      // below 2^37
            const int64_t f0 = raster_floor_div(n0, den), f1 = raster_floor_div(n1, den);
            const int64_t c0 = raster_ceil_div(n0, den), c1 = raster_ceil_div(n1, den);
            l = pl.P[j] + (f0 < f1 ? f0 : f1);
            h = pl.P[j] + (c0 > c1 ? c0 : c1);
        }
        l = (l - 1) >> 6; h = h >> 6;
        if (l < pl.lo[j]) l = pl.lo[j];
        if (h > pl.hi[j]) h = pl.hi[j];
        if (l > h) return false;
        lo[j] = l; hi[j] = h;
    }
    return true;
}

// ---- THIN ----------------------------------------------------------------------------------------------------------------------

// one axis a of one triangle: the columns (u, w) whose centres lie in the projected bounding box, clipped to the volume, the
// edges oriented by s = sign(n_a) and the plane
struct RasterThin {
    int a, u, w;
    int64_t lo[2], hi[2];      // columns, inclusive, in (u, w)
    int64_t P[3][2], d[3][2];  // edge e: its start and s (Q - P), in (u, w)
    bool tie[3];
    int64_t s, an, nu, nw, A[3];
};

// false: the triangle contributes nothing on axis a (n_a == 0, or no column centre in its box)
VRC_RASTER_HD inline bool raster_thin_setup(const int64_t v[9], const int64_t n[3], int a, uint32_t S, RasterThin& t)
{
    if (n[a] == 0) return false;
    t.a = a; t.u = (a + 1) % 3; t.w = (a + 2) % 3;
    t.s = n[a] > 0 ? 1 : -1;
    t.an = n[a] > 0 ? n[a] : -n[a];
    t.nu = n[t.u]; t.nw = n[t.w];
    for (int j = 0; j < 3; ++j) t.A[j] = v[j];
    const int ax[2] = {t.u, t.w};
    for (int i = 0; i < 2; ++i) {
        int64_t mn = v[ax[i]], mx = v[ax[i]];
        for (int k = 1; k < 3; ++k) {
            mn = v[3 * k + ax[i]] < mn ? v[3 * k + ax[i]] : mn;
            mx = v[3 * k + ax[i]] > mx ? v[3 * k + ax[i]] : mx;
        }
        t.lo[i] = (mn + 31) >> 6;                                       // ceil((mn - 32) / 64)
        t.hi[i] = (mx - 32) >> 6;                                       // floor((mx - 32) / 64)
        if (t.lo[i] < 0) t.lo[i] = 0;
        if (t.hi[i] > (int64_t)S - 1) t.hi[i] = (int64_t)S - 1;
        if (t.lo[i] > t.hi[i]) return false;
    }
    for (int e = 0; e < 3; ++e) {
        const int64_t* P = v + 3 * e;
        const int64_t* Q = v + 3 * ((e + 1) % 3);
        for (int i = 0; i < 2; ++i) {
            t.P[e][i] = P[ax[i]];
            t.d[e][i] = t.s * (Q[ax[i]] - P[ax[i]]);
        }
        t.tie[e] = t.d[e][1] > 0 || (t.d[e][1] == 0 && t.d[e][0] < 0);
    }
    return true;
}

// vrc.h's Cover rule in (u, w): the projection covers the centre of column (pu, pw)
VRC_RASTER_HD inline bool raster_covered(const RasterThin& t, int64_t pu, int64_t pw)
{
    const int64_t cu = 64 * pu + 32, cw = 64 * pw + 32;
    bool covered = true;
    for (int e = 0; e < 3; ++e) {
        const int64_t E = t.d[e][0] * (cw - t.P[e][1]) - t.d[e][1] * (cu - t.P[e][0]);
        covered = covered && (E > 0 || (E == 0 && t.tie[e]));
    }
    return covered;
}

// the voxel of a covered column that holds the crossing of its centre line with the plane (it may lie outside the volume)
VRC_RASTER_HD inline int64_t raster_thin_voxel(const RasterThin& t, int64_t pu, int64_t pw)
{
    const int64_t cu = 64 * pu + 32, cw = 64 * pw + 32;
    const int64_t M = t.an * t.A[t.a] - t.s * (t.nu * (cu - t.A[t.u]) + t.nw * (cw - t.A[t.w]));
    return raster_floor_div(M, 64 * t.an);
}

#if defined(__HIPCC__)
// n triangles (n x 9 int32, vrc.h) into the occupancy words of a volume of `depth`, mode VRC_RASTER_*; asynchronous on st
void raster_run(uint32_t* words, uint32_t depth, uint64_t n, const int32_t* tris, int mode, int solid, hipStream_t st);
#endif

}  // namespace vrc
