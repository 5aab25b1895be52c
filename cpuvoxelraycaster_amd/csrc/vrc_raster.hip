// vrc_raster.hip -- surface voxelisation of triangle meshes (include/vrc.h: vrc_raster_mesh; the rules, the pruning and
// the cost: vrc_raster.h).
//
// blockIdx.x = triangle, its work split over blockIdx.y x blockDim.x threads, as k_mark_triangles of vrc_voxelize.hip.  Neither
// mode walks the triangle's 3-D bounding box:
//   * TOUCHED: a work item is a voxel column of the projection along the dominant axis (a slab of a segment's longest axis
//     where n == 0); raster_item cuts it to the handful of voxels the plane allows, and the 13-axis predicate decides each.  The
//     13 axes depend on the triangle alone: 13 threads compute one each into LDS and every lane reads them from there.
//   * THIN: three passes of k_mark_triangles' loop, one per axis, over the projected bounding box; a covered column selects
//     one voxel.
// Selected voxels are ORed into (or ANDed out of) the occupancy word, bit layout as vrc_voxelize.hip: word = brick >> 2, bit
// (z & 1) 4 + (y & 1) 2 + (x & 1) + 8 (brick & 3).  A lane keeps the word it wrote to last and its bits, and issues the atomic
// when the next voxel falls into another word: the voxels of a column along z share a word eight at a time, those of a column
// along x or y two at a time.  One value per call, so the result does not depend on scheduling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vrc_raster.h"

namespace {

// the bits a lane has selected in one occupancy word, not yet written
struct Pending {
    uint64_t word;
    uint32_t mask;
};

__device__ __forceinline__ void flush(uint32_t* __restrict__ words, const Pending& pd, uint32_t solid)
{
    if (!pd.mask) return;
    const uint32_t have = words[pd.word];
    if (solid) { if ((have & pd.mask) != pd.mask) atomicOr(&words[pd.word], pd.mask); }
    else if (have & pd.mask) atomicAnd(&words[pd.word], ~pd.mask);
}

// voxel (x, y, z) inside the volume of (2n)^3
__device__ __forceinline__ void select_voxel(uint32_t* __restrict__ words, Pending& pd, uint32_t n, uint32_t solid, uint32_t x, uint32_t y, uint32_t z)
{
    const uint64_t brick = ((uint64_t)(x >> 1) * n + (y >> 1)) * n + (z >> 1);
    const uint32_t bit = 1u << (((z & 1u) * 4u + (y & 1u) * 2u + (x & 1u)) + 8u * (uint32_t)(brick & 3u));
    if ((brick >> 2) != pd.word) {
        flush(words, pd, solid);
        pd.word = brick >> 2; pd.mask = 0u;
    }
    pd.mask |= bit;
}

__global__ void k_raster_touched(uint32_t* __restrict__ words, uint32_t S, const int32_t* __restrict__ tris, uint32_t solid)
{
    __shared__ vrc::RasterAxis axes[13];
    const int32_t* t = tris + 9ull * blockIdx.x;
    const int32_t c[9] = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]};
    int64_t v[9];
    if (!vrc::raster_tri_kept(c, v)) return;                            // uniform for the workgroup, as the return below
    const vrc::RasterPlan pl = vrc::raster_plan(v, S);
    if (!pl.items) return;
    if (threadIdx.x < 13u) axes[threadIdx.x] = vrc::raster_axis(v, (int)threadIdx.x);
    __syncthreads();
    Pending pd = {0u, 0u};
    for (uint32_t it = blockIdx.y * blockDim.x + threadIdx.x; it < pl.items; it += gridDim.y * blockDim.x) {
        int64_t lo[3], hi[3], p[3];
        if (!vrc::raster_item(pl, axes, it, lo, hi)) continue;
        for (p[0] = lo[0]; p[0] <= hi[0]; ++p[0])
            for (p[1] = lo[1]; p[1] <= hi[1]; ++p[1])
                for (p[2] = lo[2]; p[2] <= hi[2]; ++p[2])
                    if (vrc::raster_touches(axes, p)) select_voxel(words, pd, S >> 1, solid, (uint32_t)p[0], (uint32_t)p[1], (uint32_t)p[2]);
    }
    flush(words, pd, solid);
}

__global__ void k_raster_thin(uint32_t* __restrict__ words, uint32_t S, const int32_t* __restrict__ tris, uint32_t solid)
{
    const int32_t* t = tris + 9ull * blockIdx.x;
    const int32_t c[9] = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]};
    int64_t v[9], n[3];
    if (!vrc::raster_tri_kept(c, v)) return;                            // uniform for the workgroup
    vrc::raster_normal(v, n);
    Pending pd = {0u, 0u};
    for (int a = 0; a < 3; ++a) {
        vrc::RasterThin th;
        if (!vrc::raster_thin_setup(v, n, a, S, th)) continue;          // uniform for the workgroup
        const uint32_t nw = (uint32_t)(th.hi[1] - th.lo[1] + 1);
        const uint32_t items = (uint32_t)(th.hi[0] - th.lo[0] + 1) * nw;          // at most 2^20
        for (uint32_t it = blockIdx.y * blockDim.x + threadIdx.x; it < items; it += gridDim.y * blockDim.x) {
            const int64_t pu = th.lo[0] + it / nw, pw = th.lo[1] + it % nw;
            if (!vrc::raster_covered(th, pu, pw)) continue;
            const int64_t pa = vrc::raster_thin_voxel(th, pu, pw);
            if (pa < 0 || pa >= (int64_t)S) continue;
            uint32_t p[3];
            p[th.a] = (uint32_t)pa; p[th.u] = (uint32_t)pu; p[th.w] = (uint32_t)pw;
            select_voxel(words, pd, S >> 1, solid, p[0], p[1], p[2]);
        }
    }
    flush(words, pd, solid);
}

}  // namespace

namespace vrc {

void raster_run(uint32_t* words, uint32_t depth, uint64_t n, const int32_t* tris, int mode, int solid, hipStream_t st)
{
    const uint32_t S = 1u << depth;
    // workgroups per triangle: the rule of voxelize_run (vrc_voxelize.hip) and split_for (vrc_volume.hip) -- 4096 workgroups in
    // all, at most 1024 per item -- with the S^2 columns of the largest projection for their work: keep the three in step
    uint32_t split = (uint32_t)((4096ull + n - 1) / n);
    const uint32_t useful = (S * S + 255u) / 256u;
    if (split > 1024u) split = 1024u;
    if (split > useful) split = useful;
    if (mode == VRC_RASTER_THIN)
        hipLaunchKernelGGL(k_raster_thin, dim3((uint32_t)n, split), dim3(256), 0, st, words, S, tris, solid ? 1u : 0u);
    else
        hipLaunchKernelGGL(k_raster_touched, dim3((uint32_t)n, split), dim3(256), 0, st, words, S, tris, solid ? 1u : 0u);
}

}  // namespace vrc
