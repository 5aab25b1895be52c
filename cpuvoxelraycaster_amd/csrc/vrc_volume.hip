// vrc_volume.hip -- the editable voxel volume (include/vrc.h: vrc_volume_*): the write half of the reference's
// Volumetric interface (setCell, include/volumetric.hpp:59), which LSVO leaves empty (lsvo.hpp:26).
//
// A scene stays what it is -- an immutable LNode[] that frames in flight may keep reading.  What is edited is the
// OCCUPANCY it was compiled from, resident on the device: one byte per 2 x 2 x 2 brick, [(cx*n + cy)*n + cz] with
// n = S/2, bit z*4 + y*2 + x per voxel (16 MiB at 512^3, 128 MiB at 1024^3).  That is the bottom level of the
// builder's grids in the builder's own order, and a brick byte is the child_mask / leaf_mask of its leaf parent, so a
// commit is the builder's count / rank / emit sweeps (vrc_build_sweeps.h) over a third occupancy source, BrickVox:
// bit-identical to compileSVO of the voxel set, into a NEW scene.  Batched edits are 32-bit vector atomics
// (atomicOr / atomicAnd) on the words that hold the bricks, or whole-word stores where a box covers a word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "../../include/vrc.h"
#include "vrc_build_sweeps.h"

struct vrc_volume {
    int device = 0;
    int cu_count = 0;
    uint32_t depth = 0;
    uint32_t* d_bricks = nullptr;     // n^3 brick bytes, addressed as 32-bit words by the edit kernels (n^3 is a multiple of 8)
    uint64_t n_bricks = 0;
    void* d_tex = nullptr;            // 1536 bytes: the albedo tables every committed scene gets
    unsigned long long* d_count = nullptr;
    BuildGrids grids;                 // kept between commits, allocated by the first
    // host-memory form of the edit calls: grow-only staging block
    uint32_t* d_stage = nullptr;
    size_t stage_cap = 0;
    // the last asynchronous edit: commit / download / solid_count run on the NULL stream and wait for it first
    hipEvent_t edit_done = nullptr;
    bool edit_pending = false;
};

namespace {

// ---- edits -----------------------------------------------------------------

// One thread per voxel.  All voxels of a call get the same value, so the result does not depend on the order in which
// lanes (or duplicates) arrive; out-of-volume coordinates are dropped (the rule for setCell).
__global__ void k_set_voxels(uint32_t* __restrict__ words, uint32_t S, uint64_t count, const uint32_t* __restrict__ xyz, uint32_t solid)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (x >= S || y >= S || z >= S) return;
    const uint32_t n = S >> 1;
    const uint64_t brick = ((uint64_t)(x >> 1) * n + (y >> 1)) * n + (z >> 1);
    const uint32_t bit = 1u << (((z & 1u) * 4u + (y & 1u) * 2u + (x & 1u)) + 8u * (uint32_t)(brick & 3u));
    if (solid) atomicOr(&words[brick >> 2], bit);
    else atomicAnd(&words[brick >> 2], ~bit);
}

// the voxels of brick coordinate c (one axis) that lie in [lo, hi): bit 0 = voxel 2c, bit 1 = voxel 2c + 1
__device__ __forceinline__ uint32_t axis_pair(uint32_t c, uint32_t lo, uint32_t hi)
{
    const uint32_t v = 2u * c;
    return ((v >= lo && v < hi) ? 1u : 0u) | ((v + 1u >= lo && v + 1u < hi) ? 2u : 0u);
}

// Boxes [lo, hi) clipped to the volume.  blockIdx.x = box, and the box's work is split over blockIdx.y x 256 threads.
// The work of a box is the 32-bit WORDS its brick rows touch: a row = the bricks (cx, cy, cz0..cz1), contiguous bytes;
// item = (row, k-th word of the row).  A word the box covers completely is stored as a whole (every writer of a call
// writes the same value, so a plain store next to other lanes' atomics is safe); a partly covered one is one atomic
// with the mask of the covered voxels.  Cost: proportional to the bricks inside the boxes, never to the bounding
// volume of all of them.
__global__ void k_fill_boxes(uint32_t* __restrict__ words, uint32_t S, const uint32_t* __restrict__ lo_hi, uint32_t solid)
{
    const uint32_t* b = lo_hi + 6ull * blockIdx.x;
    uint32_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = b[a];
        hi[a] = b[3 + a] < S ? b[3 + a] : S;
        if (lo[a] >= hi[a]) return;                 // empty (or wholly outside): uniform for the workgroup
    }
    const uint32_t n = S >> 1;
    const uint32_t bx0 = lo[0] >> 1, by0 = lo[1] >> 1, cz0 = lo[2] >> 1;
    const uint32_t nbx = ((hi[0] - 1u) >> 1) - bx0 + 1u, nby = ((hi[1] - 1u) >> 1) - by0 + 1u;
    const uint32_t cz1 = (hi[2] - 1u) >> 1;
    const uint32_t wpr = ((cz1 - cz0 + 3u) >> 2) + 1u;   // upper bound of the words one row touches, whatever its alignment
    const uint64_t items = (uint64_t)nbx * nby * wpr;
    for (uint64_t it = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; it < items; it += (uint64_t)gridDim.y * blockDim.x) {
        const uint32_t k = (uint32_t)(it % wpr);
        const uint32_t row = (uint32_t)(it / wpr);
        const uint32_t cx = bx0 + row / nby, cy = by0 + row % nby;
        const uint64_t base = ((uint64_t)cx * n + cy) * n;               // byte index of brick (cx, cy, 0)
        const uint64_t first = base + cz0, last = base + cz1;
        const uint64_t w = (first >> 2) + k;
        if (w > (last >> 2)) continue;
        const uint32_t xy = axis_pair(cx, lo[0], hi[0]) | (axis_pair(cy, lo[1], hi[1]) << 2);
        // xy: bit 0 / 1 = x voxel 0 / 1 inside, bit 2 / 3 = y voxel 0 / 1 inside -> the 4 (y, x) bits of one z layer
        const uint32_t layer = ((xy & 1u) ? 0x5u : 0u) | ((xy & 2u) ? 0xAu : 0u);
        const uint32_t plane = (layer & ((xy & 4u) ? 0x3u : 0u)) | (layer & ((xy & 8u) ? 0xCu : 0u));
        uint32_t mask = 0u;
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint64_t byte = 4u * w + j;
            if (byte < first || byte > last) continue;
            const uint32_t zp = axis_pair((uint32_t)(byte - base), lo[2], hi[2]);
            const uint32_t m8 = ((zp & 1u) ? plane : 0u) | ((zp & 2u) ? plane << 4 : 0u);
            mask |= m8 << (8u * j);
        }
        if (mask == 0xffffffffu) words[w] = solid ? 0xffffffffu : 0u;
        else if (mask) {
            if (solid) atomicOr(&words[w], mask);
            else atomicAnd(&words[w], ~mask);
        }
    }
}

// ---- scene -> volume ---------------------------------------------------------

// One thread per brick, descending from the root by slot (slot k = child (x = k&1, y = k>>1&1, z = k>>2), vrc.h).
// A leaf above the unit-voxel level (an array not made by compileSVO) is solid throughout.
__global__ void k_rasterise_scene(const uint2* __restrict__ nodes, uint32_t depth, uint8_t* __restrict__ bricks)
{
    const uint32_t n = 1u << (depth - 1u);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n * n * n) return;
    const uint32_t cz = (uint32_t)(i % n), cy = (uint32_t)((i / n) % n), cx = (uint32_t)(i / ((uint64_t)n * n));
    uint32_t node = 0u, value = 0u;
    uint2 rec = nodes[0];
    for (uint32_t level = 0;; ++level) {
        const uint32_t child_mask = (rec.x >> 8) & 0xffu, leaf_mask = (rec.x >> 16) & 0xffu;
        if (level + 1u == depth) { value = child_mask; break; }       // this node's children are the brick's voxels
        const uint32_t bit = depth - 2u - level;
        const uint32_t slot = ((cx >> bit) & 1u) | (((cy >> bit) & 1u) << 1) | (((cz >> bit) & 1u) << 2);
        if (!((child_mask >> slot) & 1u)) break;
        if ((leaf_mask >> slot) & 1u) { value = 0xffu; break; }
        node = node + rec.y + slot;
        rec = nodes[node];
    }
    bricks[i] = (uint8_t)value;
}

// ---- volume -> host ----------------------------------------------------------

// dense solid[(x*S + y)*S + z] bytes (the layout of vrc_build_volume_lsvo), four z-neighbours = two bricks per thread
__global__ void k_expand_dense(const uint8_t* __restrict__ bricks, uint32_t S, uint32_t* __restrict__ dense4)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t q = S >> 2, n = S >> 1;
    if (i >= (uint64_t)S * S * q) return;
    const uint32_t zq = (uint32_t)(i % q), y = (uint32_t)((i / q) % S), x = (uint32_t)(i / ((uint64_t)q * S));
    const uint8_t* p = bricks + ((uint64_t)(x >> 1) * n + (y >> 1)) * n + 2u * zq;
    const uint32_t sh = (y & 1u) * 2u + (x & 1u);
    const uint32_t b0 = p[0] >> sh, b1 = p[1] >> sh;
    dense4[i] = (b0 & 1u) | (((b0 >> 4) & 1u) << 8) | ((b1 & 1u) << 16) | (((b1 >> 4) & 1u) << 24);
}

__global__ void k_count_solid(const uint32_t* __restrict__ words, uint64_t n_words, unsigned long long* __restrict__ total)
{
    __shared__ uint32_t part[256];
    uint32_t c = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * blockDim.x)
        c += __popc(words[i]);
    part[threadIdx.x] = c;
    __syncthreads();
    for (uint32_t s = 128u; s; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0]) atomicAdd(total, (unsigned long long)part[0]);
}

void volume_free(vrc_volume* v)
{
    if (!v) return;
    (void)hipSetDevice(v->device);
    (void)hipDeviceSynchronize();       // edits may still be in flight on a caller's stream
    if (v->edit_done) (void)hipEventDestroy(v->edit_done);
    if (v->d_bricks) (void)hipFree(v->d_bricks);
    if (v->d_tex) (void)hipFree(v->d_tex);
    if (v->d_count) (void)hipFree(v->d_count);
    if (v->d_stage) (void)hipFree(v->d_stage);
    v->grids.release();
    delete v;
}

int volume_new(uint32_t depth, int device, vrc_volume** out)
{
    int cus = 0;
    int rc = vrc::require_device(device, &cus);
    if (rc) return rc;
    vrc_volume* v = new (std::nothrow) vrc_volume();
    if (!v) return vrc::fail(VRC_ERR_OOM, "out of host memory");
    v->device = device; v->cu_count = cus; v->depth = depth;
    v->n_bricks = 1ull << (3u * (depth - 1u));
    hipError_t e = hipMalloc((void**)&v->d_bricks, v->n_bricks);
    if (e == hipSuccess) e = hipMalloc(&v->d_tex, 1536);
    if (e == hipSuccess) e = hipMalloc((void**)&v->d_count, 8);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&v->edit_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemset(v->d_tex, 0xff, 1536);   // sf::Color::White, as a scene without textures
    if (e != hipSuccess) { volume_free(v); return vrc::fail_hip(e, "vrc_volume: allocation"); }
    *out = v;
    return VRC_OK;
}

// orders the NULL stream behind the last asynchronous edit
hipError_t wait_for_edits(vrc_volume* v)
{
    if (!v->edit_pending) return hipSuccess;
    v->edit_pending = false;
    return hipStreamWaitEvent(nullptr, v->edit_done, 0);
}

// Shared frame of the two edit calls: `words_per_item` u32 per item at `items`; host memory is staged and the call
// synchronous, device memory is used in place and the call asynchronous on `st`.
template <class Launch>
int edit(vrc_volume* v, const char* what, uint64_t count, uint32_t words_per_item, const uint32_t* items, int mem, hipStream_t st, Launch launch)
{
    hipError_t e = hipSetDevice(v->device);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    const uint32_t* d_items = items;
    if (mem == VRC_MEM_HOST) {
        const size_t need = (size_t)count * words_per_item * 4u;
        if (v->stage_cap < need) {
            if (v->d_stage) (void)hipFree(v->d_stage);
            v->d_stage = nullptr; v->stage_cap = 0;
            if ((e = hipMalloc((void**)&v->d_stage, need)) != hipSuccess) return vrc::fail_hip(e, what);
            v->stage_cap = need;
        }
        if ((e = hipMemcpyAsync(v->d_stage, items, need, hipMemcpyHostToDevice, st)) != hipSuccess) return vrc::fail_hip(e, what);
        d_items = v->d_stage;
    }
    launch(d_items);
    if ((e = hipGetLastError()) != hipSuccess) return vrc::fail_hip(e, what);
    if (mem == VRC_MEM_HOST) e = hipStreamSynchronize(st);
    else if (st != nullptr) { e = hipEventRecord(v->edit_done, st); v->edit_pending = true; }
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    return VRC_OK;
}

}  // namespace

extern "C" int vrc_volume_create(uint32_t depth, int device, vrc_volume** out)
{
    if (!out) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_create: null argument");
    if (depth < 2 || depth > 10) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_create: depth %u not in [2,10]", depth);
    vrc_volume* v = nullptr;
    int rc = volume_new(depth, device, &v);
    if (rc) return rc;
    hipError_t e = hipMemset(v->d_bricks, 0, v->n_bricks);
    if (e != hipSuccess) { volume_free(v); return vrc::fail_hip(e, "vrc_volume_create"); }
    *out = v;
    return VRC_OK;
}

extern "C" int vrc_volume_from_scene(const vrc_scene* s, vrc_volume** out)
{
    if (!s || !out) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_from_scene: null argument");
    if (s->depth < 2 || s->depth > 10) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_from_scene: depth %u not in [2,10]", s->depth);
    vrc_volume* v = nullptr;
    int rc = volume_new(s->depth, s->device, &v);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rasterise_scene, grid_for(v->n_bricks), dim3(256), 0, nullptr, (const uint2*)s->d_nodes, s->depth, (uint8_t*)v->d_bricks);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(v->d_tex, s->d_tex, 1536, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { volume_free(v); return vrc::fail_hip(e, "vrc_volume_from_scene"); }
    *out = v;
    return VRC_OK;
}

extern "C" int vrc_volume_destroy(vrc_volume* v)
{
    volume_free(v);
    return VRC_OK;
}

extern "C" uint32_t vrc_volume_depth(const vrc_volume* v) { return v ? v->depth : 0; }

extern "C" int vrc_volume_set_voxels(vrc_volume* v, uint64_t n, const uint32_t* xyz, int solid, int mem, void* stream)
{
    if (!v) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_set_voxels: null volume");
    if (mem != VRC_MEM_HOST && mem != VRC_MEM_DEVICE) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_set_voxels: bad mem kind %d", mem);
    if (n == 0) return VRC_OK;
    if (!xyz) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_set_voxels: null buffer");
    if (n > 0x7fffffffull * 256ull) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_set_voxels: too many voxels for one launch");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t S = 1u << v->depth;
    return edit(v, "vrc_volume_set_voxels", n, 3, xyz, mem, st, [&](const uint32_t* d_xyz) {
        hipLaunchKernelGGL(k_set_voxels, grid_for(n), dim3(256), 0, st, v->d_bricks, S, n, d_xyz, solid ? 1u : 0u);
    });
}

extern "C" int vrc_volume_fill_boxes(vrc_volume* v, uint64_t n, const uint32_t* lo_hi, int solid, int mem, void* stream)
{
    if (!v) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_fill_boxes: null volume");
    if (mem != VRC_MEM_HOST && mem != VRC_MEM_DEVICE) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_fill_boxes: bad mem kind %d", mem);
    if (n == 0) return VRC_OK;
    if (!lo_hi) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_fill_boxes: null buffer");
    if (n > 0x7fffffffull) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_fill_boxes: too many boxes for one launch");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t S = 1u << v->depth;
    // a few boxes: their words are spread over up to 1024 workgroups each (a whole 1024^3 volume is 2^25 words); many
    // boxes: one workgroup each.  A workgroup that finds nothing to do leaves at once.
    uint32_t split = (uint32_t)((4096ull + n - 1) / n);
    const uint64_t max_words = v->n_bricks / 4u;
    const uint32_t useful = (uint32_t)((max_words + 255u) / 256u);   // 256-thread groups that cover the largest possible box once
    if (split > 1024u) split = 1024u;
    if (split > useful) split = useful;
    if (split == 0) split = 1;
    return edit(v, "vrc_volume_fill_boxes", n, 6, lo_hi, mem, st, [&](const uint32_t* d_boxes) {
        hipLaunchKernelGGL(k_fill_boxes, dim3((uint32_t)n, split), dim3(256), 0, st, v->d_bricks, S, d_boxes, solid ? 1u : 0u);
    });
}

extern "C" int vrc_volume_commit(vrc_volume* v, vrc_scene** out, float* build_ms)
{
    if (!v || !out) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_commit: null argument");
    hipError_t e = hipSetDevice(v->device);
    if (e == hipSuccess) e = wait_for_edits(v);
    if (e != hipSuccess) return vrc::fail_hip(e, "vrc_volume_commit");
    vrc_scene* s = nullptr;
    const int rc = build_on_device(BrickVox{(const uint8_t*)v->d_bricks, 1u << (v->depth - 1u)}, v->depth, v->device, v->cu_count, &s, build_ms,
                                   []() { return hipSuccess; }, &v->grids);
    if (rc) return rc;
    e = hipMemcpy(s->d_tex, v->d_tex, 1536, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { vrc::scene_free(s); return vrc::fail_hip(e, "vrc_volume_commit"); }
    *out = s;
    return VRC_OK;
}

extern "C" int vrc_volume_download(vrc_volume* v, uint8_t* solid_host)
{
    if (!v || !solid_host) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_download: null argument");
    hipError_t e = hipSetDevice(v->device);
    if (e == hipSuccess) e = wait_for_edits(v);
    const uint64_t S = 1ull << v->depth;
    uint32_t* d_dense = nullptr;
    if (e == hipSuccess) e = hipMalloc((void**)&d_dense, S * S * S);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_expand_dense, grid_for(S * S * S / 4u), dim3(256), 0, nullptr, (const uint8_t*)v->d_bricks, (uint32_t)S, d_dense);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(solid_host, d_dense, S * S * S, hipMemcpyDeviceToHost);
    if (d_dense) (void)hipFree(d_dense);
    if (e != hipSuccess) return vrc::fail_hip(e, "vrc_volume_download");
    return VRC_OK;
}

extern "C" int vrc_volume_solid_count(vrc_volume* v, uint64_t* count)
{
    if (!v || !count) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_solid_count: null argument");
    hipError_t e = hipSetDevice(v->device);
    if (e == hipSuccess) e = wait_for_edits(v);
    if (e == hipSuccess) e = hipMemsetAsync(v->d_count, 0, 8, nullptr);
    if (e == hipSuccess) {
        const uint64_t n_words = v->n_bricks / 4u;
        uint64_t groups = (n_words + 255u) / 256u;
        if (groups > 4096u) groups = 4096u;
        hipLaunchKernelGGL(k_count_solid, dim3((uint32_t)groups), dim3(256), 0, nullptr, v->d_bricks, n_words, v->d_count);
        e = hipGetLastError();
    }
    unsigned long long total = 0;
    if (e == hipSuccess) e = hipMemcpy(&total, v->d_count, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return vrc::fail_hip(e, "vrc_volume_solid_count");
    *count = total;
    return VRC_OK;
}
