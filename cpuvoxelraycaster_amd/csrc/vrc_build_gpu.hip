// vrc_build_gpu.hip -- LSVO construction on the GPU: the step
// immediately before the hot path.  Produces, directly in HBM, the exact array
// compileSVO emits (src/lsvo_utils.cpp:4-49 over the tree SVO::setCell builds,
// include/svo.hpp:72-114) -- bit-identical to the host builder and to the oracle.
//
// The count / rank / emit sweeps themselves are in vrc_build_sweeps.h (shared with the editable volume,
// vrc_volume.hip); this file holds the occupancy sources of the one-shot builds and the terrain noise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>
#include <random>
#include <vector>

#include "../../include/vrc.h"
#include "vrc_build_sweeps.h"

namespace {

// voxel occupancy sources ----------------------------------------------------

// main.cpp:65-74: column (x,z) solid for y in [S/2 + 1, S/2 + lim), lim = max(16, min(S, height));
// voxels outside the volume are dropped (out-of-bounds Node::sub index in the reference).
struct TerrainVox {
    const int32_t* lim;  // [x*S + z]
    uint32_t S;
    __device__ bool operator()(uint32_t x, uint32_t y, uint32_t z) const
    {
        const int32_t base = (int32_t)(S / 2u);
        const int32_t l = lim[(size_t)x * S + z];
        return (int32_t)y >= base + 1 && (int32_t)y < base + l;
    }
};

struct VolumeVox {
    const uint8_t* solid;  // [(x*S + y)*S + z]
    uint32_t S;
    __device__ bool operator()(uint32_t x, uint32_t y, uint32_t z) const
    {
        return solid[((size_t)x * S + y) * S + z] != 0;
    }
};

__global__ void k_terrain_lim(const int32_t* __restrict__ height, int32_t* __restrict__ lim, uint32_t S)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * S) return;
    int32_t l = height[i];
    if (l > (int32_t)S) l = (int32_t)S;   // std::min(max_height, height)
    if (l < 16) l = 16;                   // std::max(ground_level, ...)
    lim[i] = l;
}

}  // namespace

// ---------------------------------------------------------------------------
// N4: the terrain generator's noise (src/main.cpp:61-69 over the vendored
// FastNoise v0.4.1, SimplexFractal / FBM, FN_DECIMAL = float) on the GPU, so the
// whole chain noise -> heights -> LSVO -> frames stays in HBM.  Bit-identical to
// the real FastNoise (tests compare with heights produced by the reference's own
// FastNoise.cpp).  All float operations in the reference's order, no contraction.
//
// The noise ALGORITHM restated here (seeded permutation, 2-D simplex, FBM) is FastNoise's:
//   FastNoise -- MIT License -- Copyright (c) 2017 Jordan Peck
//   Permission is hereby granted, free of charge, to any person obtaining a copy of this software and associated
//   documentation files (the "Software"), to deal in the Software without restriction, including without limitation
//   the rights to use, copy, modify, merge, publish, distribute, sublicense, and/or sell copies of the Software,
//   and to permit persons to whom the Software is furnished to do so, subject to the following conditions: The
//   above copyright notice and this permission notice shall be included in all copies or substantial portions of
//   the Software.  THE SOFTWARE IS PROVIDED "AS IS", WITHOUT WARRANTY OF ANY KIND.
// ---------------------------------------------------------------------------
namespace {

struct NoiseTables {
    uint8_t perm[512], perm12[512];
    float F2, G2, two_G2, bounding;
};

// The permutation the reference's FastNoise builds for a seed (FastNoise::SetSeed, FastNoise.cpp:197-215): a
// Fisher-Yates pass over the identity, position `done` drawing its partner from the not yet fixed tail with
// std::mt19937_64 (one draw per position, modulo the tail length); both tables are stored twice so that
// perm[a + perm[b]] needs no wrap.  Plus the 2-D simplex skew constants (:1270-1272) and the FBM normaliser
// (CalculateFractalBounding, :217-227: gain 0.5, 3 octaves).  Host side.
void noise_tables(int seed, NoiseTables& t)
{
    std::mt19937_64 draw(seed);
    uint8_t order[256];
    for (unsigned v = 0; v < 256u; ++v) order[v] = (uint8_t)v;
    for (unsigned done = 0; done < 256u; ++done) {
        const unsigned pick = done + (unsigned)((int)(draw() % (256u - done)));
        const uint8_t fixed = order[pick];
        order[pick] = order[done];
        order[done] = fixed;
    }
    for (unsigned v = 0; v < 256u; ++v) {
        t.perm[v] = t.perm[v + 256u] = order[v];
        t.perm12[v] = t.perm12[v + 256u] = (uint8_t)(order[v] % 12u);
    }
    const volatile float root3 = 1.7320508075688772935274463415059f;
    t.F2 = 0.5f * (root3 - 1.0f);
    t.G2 = (3.0f - root3) / 6.0f;
    t.two_G2 = 2.0f * t.G2;
    float octave_gain = 0.5f, total = 1.0f;                // 1 + 0.5 + 0.25
    for (int octave = 1; octave < 3; ++octave) { total += octave_gain; octave_gain *= 0.5f; }
    t.bounding = 1.0f / total;
}

__device__ __forceinline__ int fn_fast_floor(float f) { return f >= 0 ? (int)f : (int)f - 1; }   // FastNoise.cpp:184

// One simplex corner's term: falloff (0.5 - |d|^2)^4 times the gradient picked by the doubly indexed permutation
// (Index2D_12, FastNoise.cpp:244-247; GradCoord2D, :312-317).  The 12 gradients (GRAD_X / GRAD_Y, :37-48, two
// tables there) are decoded from the index instead: entries 0-3 are the four diagonals (+-1, +-1), 4-7 are
// (+-1, 0) and 8-11 are (0, +-1), the sign alternating with the index.  A corner outside the falloff radius
// contributes exactly +0.
__device__ __forceinline__ float fn_corner2(const uint8_t* perm, const uint8_t* perm12, uint32_t offset, int cell_x, int cell_y,
                                            float dx, float dy)
{
    float fall = 0.5f - dx * dx - dy * dy;
    if (fall < 0) return 0.0f;
    const uint32_t g = perm12[(cell_x & 0xff) + perm[(cell_y & 0xff) + offset]];
    const float odd = (g & 1u) ? -1.0f : 1.0f;
    const float gx = g >= 8u ? 0.0f : odd;
    const float gy = g >= 8u ? odd : (g >= 4u ? 0.0f : ((g & 2u) ? -1.0f : 1.0f));
    fall *= fall;
    return fall * fall * (dx * gx + dy * gy);
}

// 2-D simplex noise of one octave (SingleSimplex, FastNoise.cpp:1274-1335): skew the point onto the lattice of
// unit cells, un-skew the cell origin, and sum the terms of the triangle's three corners -- the origin, the
// middle corner (one step along the larger of the two offsets), and the far corner (1, 1).
__device__ float fn_simplex2(const uint8_t* perm, const uint8_t* perm12, uint32_t offset, float x, float y, float F2, float G2, float two_G2)
{
    const float skew = (x + y) * F2;
    const int cell_x = fn_fast_floor(x + skew), cell_y = fn_fast_floor(y + skew);
    const float unskew = (float)(cell_x + cell_y) * G2;
    const float ox = x - ((float)cell_x - unskew), oy = y - ((float)cell_y - unskew);   // offset from the cell origin
    const int step_x = ox > oy ? 1 : 0, step_y = 1 - step_x;
    float sum = fn_corner2(perm, perm12, offset, cell_x, cell_y, ox, oy);
    sum = sum + fn_corner2(perm, perm12, offset, cell_x + step_x, cell_y + step_y, ox - (float)step_x + G2, oy - (float)step_y + G2);
    sum = sum + fn_corner2(perm, perm12, offset, cell_x + 1, cell_y + 1, ox - 1.0f + two_G2, oy - 1.0f + two_G2);
    return 70.0f * sum;
}

__global__ void k_terrain_heights(NoiseTables tab, uint32_t S, int32_t* __restrict__ height)
{
    __shared__ uint8_t perm[512], perm12[512];
    for (uint32_t i = threadIdx.x; i < 512u; i += blockDim.x) { perm[i] = tab.perm[i]; perm12[i] = tab.perm12[i]; }
    __syncthreads();
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= S * S) return;
    const uint32_t x = idx / S, z = idx % S;
    // GetNoise(0.75 x, 0.75 z): frequency 0.01, FBM over 3 octaves, lacunarity 2, gain 0.5 (:410-447, :1175-1207)
    float fx = (0.75f * (float)x) * 0.01f, fy = (0.75f * (float)z) * 0.01f;
    float sum = fn_simplex2(perm, perm12, perm[0], fx, fy, tab.F2, tab.G2, tab.two_G2);
    float amp = 1.0f;
    for (int o = 1; o < 3; ++o) {
        fx *= 2.0f; fy *= 2.0f;
        amp *= 0.5f;
        sum += fn_simplex2(perm, perm12, perm[o], fx, fy, tab.F2, tab.G2, tab.two_G2) * amp;
    }
    const float noise = sum * tab.bounding;
    height[idx] = (int32_t)(64.0f * noise + 32.0f);                              // main.cpp:69
}

}  // namespace

extern "C" int vrc_terrain_heights(int32_t seed, uint32_t size, int device, int32_t* height_host)
{
    if (!height_host || size == 0 || size > 4096) return vrc::fail(VRC_ERR_INVALID, "vrc_terrain_heights: bad argument");
    int rc = vrc::require_device(device, nullptr);
    if (rc) return rc;
    NoiseTables tab;
    noise_tables(seed, tab);
    int32_t* d_h = nullptr;
    hipError_t e = hipMalloc((void**)&d_h, (size_t)size * size * 4);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_terrain_heights, grid_for((uint64_t)size * size), dim3(256), 0, nullptr, tab, size, d_h);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(height_host, d_h, (size_t)size * size * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_h);
    if (e != hipSuccess) return vrc::fail_hip(e, "vrc_terrain_heights");
    return VRC_OK;
}

// main.cpp:59-88 end to end on the device: noise -> column limits -> LSVO.
extern "C" int vrc_scene_build_fastnoise_terrain(int32_t seed, uint32_t depth, int device, vrc_scene** out, float* build_ms)
{
    if (!out) return vrc::fail(VRC_ERR_INVALID, "vrc_scene_build_fastnoise_terrain: null argument");
    if (depth < 2 || depth > 10) return vrc::fail(VRC_ERR_INVALID, "vrc_scene_build_fastnoise_terrain: depth %u not in [2,10]", depth);
    int cus = 0;
    int rc = vrc::require_device(device, &cus);
    if (rc) return rc;
    const uint32_t S = 1u << depth;
    NoiseTables tab;
    noise_tables(seed, tab);
    int32_t *d_h = nullptr, *d_lim = nullptr;
    hipError_t e = hipMalloc((void**)&d_h, (size_t)S * S * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d_lim, (size_t)S * S * 4);
    if (e != hipSuccess) rc = vrc::fail_hip(e, "vrc_scene_build_fastnoise_terrain");
    else rc = build_on_device(TerrainVox{d_lim, S}, depth, device, cus, out, build_ms, [&]() {
        // inside the timed region: *build_ms covers noise -> heights -> column limits -> LSVO
        hipLaunchKernelGGL(k_terrain_heights, grid_for((uint64_t)S * S), dim3(256), 0, nullptr, tab, S, d_h);
        hipLaunchKernelGGL(k_terrain_lim, grid_for((uint64_t)S * S), dim3(256), 0, nullptr, d_h, d_lim, S);
        return hipGetLastError();
    });
    (void)hipFree(d_h);
    (void)hipFree(d_lim);
    return rc;
}

extern "C" int vrc_scene_build_terrain(const int32_t* height, uint32_t depth, int device, vrc_scene** out, float* build_ms)
{
    if (!height || !out) return vrc::fail(VRC_ERR_INVALID, "vrc_scene_build_terrain: null argument");
    if (depth < 2 || depth > 10) return vrc::fail(VRC_ERR_INVALID, "vrc_scene_build_terrain: depth %u not in [2,10]", depth);
    int cus = 0;
    int rc = vrc::require_device(device, &cus);
    if (rc) return rc;
    const uint32_t S = 1u << depth;
    int32_t *d_h = nullptr, *d_lim = nullptr;
    hipError_t e = hipMalloc((void**)&d_h, (size_t)S * S * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d_lim, (size_t)S * S * 4);
    if (e == hipSuccess) e = hipMemcpy(d_h, height, (size_t)S * S * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = vrc::fail_hip(e, "vrc_scene_build_terrain");
    else rc = build_on_device(TerrainVox{d_lim, S}, depth, device, cus, out, build_ms, [&]() {
        hipLaunchKernelGGL(k_terrain_lim, grid_for((uint64_t)S * S), dim3(256), 0, nullptr, d_h, d_lim, S);
        return hipGetLastError();
    });
    (void)hipFree(d_h);
    (void)hipFree(d_lim);
    return rc;
}

extern "C" int vrc_scene_build_volume(const uint8_t* solid, uint32_t depth, int device, vrc_scene** out, float* build_ms)
{
    if (!solid || !out) return vrc::fail(VRC_ERR_INVALID, "vrc_scene_build_volume: null argument");
    if (depth < 2 || depth > 10) return vrc::fail(VRC_ERR_INVALID, "vrc_scene_build_volume: depth %u not in [2,10]", depth);
    int cus = 0;
    int rc = vrc::require_device(device, &cus);
    if (rc) return rc;
    const uint64_t S = 1ull << depth;
    uint8_t* d_solid = nullptr;
    hipError_t e = hipMalloc((void**)&d_solid, S * S * S);
    if (e == hipSuccess) e = hipMemcpy(d_solid, solid, S * S * S, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = vrc::fail_hip(e, "vrc_scene_build_volume");
    else rc = build_on_device(VolumeVox{d_solid, (uint32_t)S}, depth, device, cus, out, build_ms, []() { return hipSuccess; });
    (void)hipFree(d_solid);
    return rc;
}

extern "C" int vrc_scene_download_nodes(const vrc_scene* s, vrc_lnode* dst)
{
    if (!s || !dst) return vrc::fail(VRC_ERR_INVALID, "vrc_scene_download_nodes: null argument");
    hipError_t e = hipSetDevice(s->device);
    if (e == hipSuccess) e = hipMemcpy(dst, s->d_nodes, s->n_nodes * sizeof(vrc_lnode), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return vrc::fail(VRC_ERR_HIP, "vrc_scene_download_nodes: %s", hipGetErrorString(e));
    return VRC_OK;
}
