// vrc_build_sweeps.h -- the count / rank / emit sweeps of the GPU LSVO builder, shared by the
// translation units that bring an occupancy source of their own: vrc_build_gpu.hip (terrain columns,
// dense byte volume) and vrc_volume.hip (the editable brick volume, vrc_volume_commit).
//
// The layout is a depth-first pre-order: the k-th node visited by compileSVO_rec
// (k = 0 for the root) owns the 8 slots starting at 1 + 8k, and a node's own
// index is its parent's block + slot (lsvo_utils.cpp:8-10,25-27,37-39).  With
//   cnt(v)  = number of internal (non-leaf, non-empty) nodes in v's subtree,
//   rank(v) = pre-order index of v among internal nodes
//           = rank(parent) + 1 + sum of cnt over the siblings visited before v,
// where siblings are visited x-outer, y-middle, z-inner (:29-31) and written to
// slot z*4 + y*2 + x (:34), the whole array follows from two sweeps over dense
// per-level grids: counts bottom-up, ranks + node records top-down.  Integer /
// byte work, HBM-bound; no MFMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "../../include/vrc.h"
#include "vrc_build_grids.h"
#include "vrc_host.h"

namespace {

#define HIP_TRYB(expr)                                                                              \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess) { rc = vrc::fail_hip(e_, #expr); goto done; }                         \
    } while (0)

// An occupancy source is a functor vox(x, y, z) -> bool in SVO::setCell coordinates.  The sweeps only ever ask for
// the eight voxels of one 2 x 2 x 2 brick at a time: bit z*4 + y*2 + x (the slot of lsvo_utils.cpp:34) per voxel.
template <class Vox>
__device__ __forceinline__ uint32_t brick_mask(const Vox& vox, uint32_t cx, uint32_t cy, uint32_t cz)
{
    uint32_t m = 0u;
    for (uint32_t x = 0; x < 2; ++x)                // visiting order of lsvo_utils.cpp:29-31
        for (uint32_t y = 0; y < 2; ++y)
            for (uint32_t z = 0; z < 2; ++z)
                if (vox(2 * cx + x, 2 * cy + y, 2 * cz + z)) m |= 1u << (z * 4u + y * 2u + x);
    return m;
}

// The editable volume (vrc_volume.hip): one byte per brick, [(cx*n + cy)*n + cz] with n = S/2 bricks per axis, in
// exactly that bit order -- a brick byte IS the child_mask / leaf_mask of its leaf parent, one load instead of eight.
struct BrickVox {
    const uint8_t* bricks;
    uint32_t n;
    __device__ bool operator()(uint32_t x, uint32_t y, uint32_t z) const
    {
        const uint32_t b = bricks[((size_t)(x >> 1) * n + (y >> 1)) * n + (z >> 1)];
        return (b >> ((z & 1u) * 4u + (y & 1u) * 2u + (x & 1u))) & 1u;
    }
};
__device__ __forceinline__ uint32_t brick_mask(const BrickVox& vox, uint32_t cx, uint32_t cy, uint32_t cz)
{
    return vox.bricks[((size_t)cx * vox.n + cy) * vox.n + cz];
}

// level N-1 (parents of unit voxels): cnt = 1 if any of the 8 voxels is solid
template <class Vox>
__global__ void k_count_leaf_parents(Vox vox, uint32_t n /* cells per axis */, uint32_t* __restrict__ cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n * n * n) return;
    const uint32_t cz = (uint32_t)(i % n), cy = (uint32_t)((i / n) % n), cx = (uint32_t)(i / ((uint64_t)n * n));
    cnt[i] = brick_mask(vox, cx, cy, cz) ? 1u : 0u;
}

// level L < N-1: cnt = 1 + sum of the children's counts if any child exists
__global__ void k_count_level(const uint32_t* __restrict__ child_cnt, uint32_t n, uint32_t* __restrict__ cnt)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n * n * n) return;
    const uint32_t cz = (uint32_t)(i % n), cy = (uint32_t)((i / n) % n), cx = (uint32_t)(i / ((uint64_t)n * n));
    const uint32_t m = 2 * n;
    uint32_t s = 0;
    for (uint32_t k = 0; k < 8; ++k)
        s += child_cnt[((uint64_t)(2 * cx + (k >> 2)) * m + (2 * cy + ((k >> 1) & 1))) * m + (2 * cz + (k & 1))];
    cnt[i] = s ? s + 1u : 0u;
}

// top-down: write this level's node records, hand rank / index to the children.
// LEAF_LEVEL: children are unit voxels (leaf_mask, lsvo_utils.cpp:40-42).
template <class Vox, bool LEAF_LEVEL>
__global__ void k_emit_level(Vox vox, uint32_t n, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ child_cnt,
                             const uint32_t* __restrict__ rank, const uint32_t* __restrict__ index,
                             uint32_t* __restrict__ child_rank, uint32_t* __restrict__ child_index,
                             uint2* __restrict__ nodes)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n * n * n) return;
    if (cnt[i] == 0u) return;                       // empty cell: its slot keeps the blank LNode()
    const uint32_t cz = (uint32_t)(i % n), cy = (uint32_t)((i / n) % n), cx = (uint32_t)(i / ((uint64_t)n * n));
    const uint32_t m = 2 * n;
    const uint32_t my_rank = rank[i], my_index = index[i];
    const uint32_t block = 1u + 8u * my_rank;       // child_pos = data.size() at visit time (:8)
    uint32_t child_mask = 0u, leaf_mask = 0u;
    if (LEAF_LEVEL) {
        child_mask = leaf_mask = brick_mask(vox, cx, cy, cz);
    } else {
        uint32_t running = my_rank + 1u;
        for (uint32_t x = 0; x < 2; ++x)            // visiting order of lsvo_utils.cpp:29-31
            for (uint32_t y = 0; y < 2; ++y)
                for (uint32_t z = 0; z < 2; ++z) {
                    const uint32_t sub_index = z * 4u + y * 2u + x;   // :34
                    const uint64_t ci = ((uint64_t)(2 * cx + x) * m + (2 * cy + y)) * m + (2 * cz + z);
                    const uint32_t c = child_cnt[ci];
                    if (c) {
                        child_mask |= 1u << sub_index;
                        child_rank[ci] = running;
                        child_index[ci] = block + sub_index;
                        running += c;
                    }
                }
    }
    // LNode{color 1, child_mask, leaf_mask, pad 0, child_offset} (lsvo_utils.hpp:5-18)
    nodes[my_index] = make_uint2(1u | (child_mask << 8) | (leaf_mask << 16), block - my_index);
}

__global__ void k_fill_blank_nodes(uint2* __restrict__ nodes, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) nodes[i] = make_uint2(1u, 0u);       // LNode(): color 1, everything else 0
}

inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// `pre` (optional) enqueues the kernels that produce the occupancy source (noise, column limits); it runs inside the
// timed region.  *ms_out = device time of the build: [pre + count sweep] + [blank fill + emit sweep], two event
// pairs around the enqueued kernels; the per-level grids are allocated before the first event (or come from the
// caller: `keep`, allocated here on first use and left to its owner), and the node array's allocation (its size is
// the count sweep's result) lies between the pairs -- neither is timed.  Runs on the NULL stream; synchronous.
template <class Vox, class Pre>
int build_on_device(Vox vox, uint32_t depth, int device, int cus, vrc_scene** out, float* ms_out, Pre pre, BuildGrids* keep = nullptr)
{
    int rc = VRC_OK;
    const uint32_t N = depth;
    BuildGrids own;
    BuildGrids& g = keep ? *keep : own;
    void* d_nodes = nullptr;
    void* d_tex = nullptr;
    vrc_scene* s = nullptr;
    uint32_t root_cnt = 0;
    uint64_t n_nodes = 0;
    float ms_count = 0.0f, ms_emit = 0.0f;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; ++i) HIP_TRYB(hipEventCreate(&ev[i]));
    if (!g.allocated()) {
        const hipError_t ea = g.alloc(N);
        if (ea != hipSuccess) g.release();
        HIP_TRYB(ea);
    }
    HIP_TRYB(hipMemsetAsync(g.rank[0], 0, 4, nullptr));
    HIP_TRYB(hipMemsetAsync(g.index[0], 0, 4, nullptr));
    HIP_TRYB(hipEventRecord(ev[0], nullptr));
    HIP_TRYB(pre());
    // bottom-up counts
    {
        const uint32_t n = 1u << (N - 1);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_count_leaf_parents<Vox>), grid_for((uint64_t)n * n * n), dim3(256), 0, nullptr, vox, n, g.cnt[N - 1]);
        for (int L = (int)N - 2; L >= 0; --L) {
            const uint32_t nl = 1u << L;
            hipLaunchKernelGGL(k_count_level, grid_for((uint64_t)nl * nl * nl), dim3(256), 0, nullptr, g.cnt[L + 1], nl, g.cnt[L]);
        }
        HIP_TRYB(hipGetLastError());
    }
    HIP_TRYB(hipEventRecord(ev[1], nullptr));
    HIP_TRYB(hipMemcpy(&root_cnt, g.cnt[0], 4, hipMemcpyDeviceToHost));
    n_nodes = 1ull + 8ull * root_cnt;                 // data = { root } + 8 slots per internal node
    if (n_nodes > VRC_MAX_NODES) { rc = vrc::fail(VRC_ERR_INVALID, "scene needs more than 2^29 nodes (4 GiB)"); goto done; }
    HIP_TRYB(hipMalloc(&d_nodes, n_nodes * sizeof(vrc_lnode)));
    HIP_TRYB(hipMalloc(&d_tex, 1536));
    HIP_TRYB(hipEventRecord(ev[2], nullptr));
    hipLaunchKernelGGL(k_fill_blank_nodes, grid_for(n_nodes), dim3(256), 0, nullptr, (uint2*)d_nodes, n_nodes);
    if (root_cnt == 0) {
        // empty scene: compileSVO_rec still stores child_offset = 1 in the root (:8-10) and appends nothing
        const vrc_lnode root = {1u, 0u, 0u, 0u, 1u};
        HIP_TRYB(hipMemcpy(d_nodes, &root, sizeof(root), hipMemcpyHostToDevice));
    } else {
        for (uint32_t L = 0; L < N; ++L) {
            const uint32_t n = 1u << L;
            const uint64_t cells = (uint64_t)n * n * n;
            if (L + 1 == N)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_emit_level<Vox, true>), grid_for(cells), dim3(256), 0, nullptr, vox, n, g.cnt[L],
                                   (const uint32_t*)nullptr, g.rank[L], g.index[L], (uint32_t*)nullptr, (uint32_t*)nullptr, (uint2*)d_nodes);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_emit_level<Vox, false>), grid_for(cells), dim3(256), 0, nullptr, vox, n, g.cnt[L],
                                   g.cnt[L + 1], g.rank[L], g.index[L], g.rank[L + 1], g.index[L + 1], (uint2*)d_nodes);
        }
        HIP_TRYB(hipGetLastError());
    }
    HIP_TRYB(hipEventRecord(ev[3], nullptr));
    HIP_TRYB(hipEventSynchronize(ev[3]));
    HIP_TRYB(hipEventElapsedTime(&ms_count, ev[0], ev[1]));
    HIP_TRYB(hipEventElapsedTime(&ms_emit, ev[2], ev[3]));
    if (ms_out) *ms_out = ms_count + ms_emit;
    HIP_TRYB(hipMemset(d_tex, 0xff, 1536));
    s = new (std::nothrow) vrc_scene();
    if (!s) { rc = vrc::fail(VRC_ERR_OOM, "out of host memory"); goto done; }
    s->device = device; s->cu_count = cus; s->d_nodes = d_nodes; s->d_tex = d_tex; s->n_nodes = n_nodes; s->depth = depth;
    d_nodes = nullptr; d_tex = nullptr;
    *out = s;
done:
    own.release();
    if (d_nodes) (void)hipFree(d_nodes);
    if (d_tex) (void)hipFree(d_tex);
    for (int i = 0; i < 4; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
    return rc;
}

}  // namespace
