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
//
// Here: the volume's life cycle, the edits and queries on the occupancy with their ordering and scratch blocks, and
// commit / download.  Boxes, spheres, spheres at the hits of a ray batch, region copies and the two queries have their
// kernels here, over the box-of-words layout of vrc_box_words.h.  The other features keep theirs in files of their own:
// vrc_flood.hip, vrc_voxelize.hip, vrc_surface.hip, vrc_voxels.hip, vrc_rects.hip, vrc_stamp.hip, vrc_pack.hip, vrc_stroke.hip,
// vrc_raster.hip.  The calls between two volumes and along their axes (cells, columns, levels, morphology) are in
// vrc_volume_ops.hip, the snapshots taken from a volume (labels, fields, deltas) in vrc_snapshots.hip; what the entry points of
// the three files share -- the checks, the ordering rule and staged_call, the one frame of every call -- is in
// vrc_volume_state.h, and the ordering of every entry point is the table in DESIGN.md.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <new>

#include "../../include/vrc.h"
#include "vrc_box_words.h"
#include "vrc_build_sweeps.h"
#include "vrc_flood.h"
#include "vrc_group.h"
#include "vrc_pack.h"
#include "vrc_raster.h"
#include "vrc_stamp.h"
#include "vrc_stroke.h"
#include "vrc_rects.h"
#include "vrc_surface.h"
#include "vrc_volume_state.h"
#include "vrc_voxelize.h"
#include "vrc_voxels.h"

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
    const uint64_t brick = brick_of(S >> 1, x, y, z);
    const uint32_t bit = 1u << (voxel_bit(x, y, z) + 8u * (uint32_t)(brick & 3u));
    if (solid) atomicOr(&words[brick >> 2], bit);
    else atomicAnd(&words[brick >> 2], ~bit);
}

// Boxes [lo, hi) clipped to the volume.  blockIdx.x = box, and the box's work is split over blockIdx.y x 256 threads.
// The work of a box is the 32-bit WORDS its brick rows touch (BoxWords).  A word the box covers completely is stored as
// a whole (every writer of a call writes the same value, so a plain store next to other lanes' atomics is safe); a
// partly covered one is one atomic with the mask of the covered voxels.  Cost: proportional to the bricks inside the
// boxes, never to the bounding volume of all of them.
__global__ void k_fill_boxes(uint32_t* __restrict__ words, uint32_t S, const uint32_t* __restrict__ lo_hi, uint32_t solid)
{
    uint32_t lo[3], hi[3];
    if (!clip_box(lo_hi + 6ull * blockIdx.x, S, lo, hi)) return;      // uniform for the workgroup
    const uint32_t n = S >> 1;
    const BoxWords b = box_words(lo, hi);
    for (uint64_t it = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; it < b.items; it += (uint64_t)gridDim.y * blockDim.x) {
        RowWord r;
        if (!row_word(b, n, it, r)) continue;
        const uint32_t mask = box_mask(b, r);
        if (mask == 0xffffffffu) words[r.w] = solid ? 0xffffffffu : 0u;
        else if (mask) {
            if (solid) atomicOr(&words[r.w], mask);
            else atomicAnd(&words[r.w], ~mask);
        }
    }
}

// ---- brushes -----------------------------------------------------------------

#define VRC_BRUSH_LIMIT (1 << 20)     // |centre| and radius of a sphere: squares and their sums stay far inside 64 bits

// floor(sqrt(v)) for 0 <= v <= 2^42, exact: the double root is within one of it
__device__ __forceinline__ int64_t isqrt(int64_t v)
{
    int64_t h = (int64_t)sqrt((double)v);
    while (h * h > v) --h;
    while ((h + 1) * (h + 1) <= v) ++h;
    return h;
}

// Spheres (cx, cy, cz, r): voxel (x, y, z) belongs iff dx^2 + dy^2 + dz^2 <= r^2 in integers.  blockIdx.x = sphere, its
// work split over blockIdx.y x blockDim.x threads and laid out as the words of its OWN bounding box clipped to the
// volume (BoxWords), so the cost follows the bricks around each sphere, never the volume or the batch's bounding volume.
// A voxel column (x, y) of a sphere is one z interval, cz -/+ isqrt(r^2 - dx^2 - dy^2): a word's mask follows from the
// four intervals of its brick row.  Whole words are stored, partly covered ones take one atomic -- none at all where the
// word already has the value (all writers of a call write the same value, so a stale read only costs the atomic; the
// hits of neighbouring rays name the same voxels over and over).
__global__ void k_fill_spheres(uint32_t* __restrict__ words, uint32_t S, const int32_t* __restrict__ centre_radius, uint32_t solid)
{
    const int32_t* s = centre_radius + 4ull * blockIdx.x;
    const int32_t c[3] = {s[0], s[1], s[2]}, rad = s[3];
    if (rad < 0 || rad > VRC_BRUSH_LIMIT) return;                      // uniform for the workgroup, as every return below
    uint32_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        if (c[a] > VRC_BRUSH_LIMIT || c[a] < -VRC_BRUSH_LIMIT) return;
        const int32_t l = c[a] - rad, h = c[a] + rad + 1;              // |.| <= 2^21 + 1
        if (h <= 0 || l >= (int32_t)S) return;
        lo[a] = l < 0 ? 0u : (uint32_t)l;
        hi[a] = h > (int32_t)S ? S : (uint32_t)h;
    }
    const uint32_t n = S >> 1;
    const int64_t r2 = (int64_t)rad * rad;
    const BoxWords b = box_words(lo, hi);
    for (uint64_t it = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; it < b.items; it += (uint64_t)gridDim.y * blockDim.x) {
        RowWord r;
        if (!row_word(b, n, it, r)) continue;
        // the z interval [zl, zh] of each of the row's four columns, k = y * 2 + x as in a brick's bit index
        int32_t zl[4], zh[4];
        bool any = false;
        for (int k = 0; k < 4; ++k) {
            const int64_t dx = (int64_t)(2u * r.cx + (k & 1)) - c[0], dy = (int64_t)(2u * r.cy + (k >> 1)) - c[1];
            const int64_t rem = r2 - dx * dx - dy * dy;
            if (rem < 0) { zl[k] = 1; zh[k] = 0; continue; }
            const int32_t h = (int32_t)isqrt(rem);
            zl[k] = c[2] - h; zh[k] = c[2] + h;
            any = true;
        }
        if (!any) continue;
        uint32_t mask = 0u;
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint64_t byte = 4u * r.w + j;
            if (byte < r.first || byte > r.last) continue;
            const int32_t z0 = 2 * (int32_t)(byte - r.base);
            uint32_t m8 = 0u;
            for (int k = 0; k < 4; ++k)
                m8 |= ((z0 >= zl[k] && z0 <= zh[k]) ? 1u << k : 0u) | ((z0 + 1 >= zl[k] && z0 + 1 <= zh[k]) ? 16u << k : 0u);
            mask |= m8 << (8u * j);
        }
        if (mask == 0xffffffffu) words[r.w] = solid ? 0xffffffffu : 0u;
        else if (mask) {
            const uint32_t have = words[r.w];
            if (solid) { if ((have & mask) != mask) atomicOr(&words[r.w], mask); }
            else if (have & mask) atomicAnd(&words[r.w], ~mask);
        }
    }
}

// vrc_hit_to_voxel (vrc_api.cpp) per record, the same float32 operations: centre = the voxel hit (dig) or the empty
// cell the ray came through (build); records that function refuses, and a build without a neighbour, get radius -1,
// which k_fill_spheres drops.
__global__ void k_hits_to_centres(uint64_t count, const vrc_hit* __restrict__ hits, uint32_t depth, int32_t radius, uint32_t build,
                                  int32_t* __restrict__ centre_radius)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const vrc_hit h = hits[i];
    const int32_t Si = (int32_t)(1u << depth);
    const float S = (float)Si;
    int32_t cell[3];
    bool ok = (h.hit & 0xffu) == 1u;
    for (int a = 0; a < 3; ++a) {
        const float f = floorf((h.position[a] - 1.0f) * S);
        ok = ok && f >= 0.0f && f < S;                                  // NaN fails both
        cell[a] = ok ? Si - 1 - (int32_t)f : 0;
    }
    if (ok && build) {
        int axis = -1, axes = 0;
        for (int a = 0; a < 3; ++a) if (h.normal[a] != 0.0f) { axis = a; ++axes; }
        ok = axes == 1;
        if (ok) {
            cell[axis] -= h.normal[axis] > 0.0f ? 1 : -1;
            ok = cell[axis] >= 0 && cell[axis] < Si;
        }
    }
    int4 out;
    out.x = cell[0]; out.y = cell[1]; out.z = cell[2]; out.w = ok ? radius : -1;
    ((int4*)centre_radius)[i] = out;
}

// ---- region copy ---------------------------------------------------------------

// bit k = voxel (x, y, z0 + k) of the source, 0 <= k < 10 where the voxel exists: the column's bits of the five bricks
// from z0 on (z0 even, may be negative or beyond the volume)
__device__ __forceinline__ uint32_t source_column(const uint8_t* __restrict__ src, uint32_t ns, int64_t x, int64_t y, int64_t z0)
{
    const int64_t Ss = 2 * (int64_t)ns;
    if (x < 0 || y < 0 || x >= Ss || y >= Ss) return 0u;
    const uint8_t* row = src + ((uint64_t)(x >> 1) * ns + (uint64_t)(y >> 1)) * ns;
    const uint32_t sh = (uint32_t)(y & 1) * 2u + (uint32_t)(x & 1);
    uint32_t bits = 0u;
    for (int j = 0; j < 5; ++j) {
        const int64_t bz = (z0 >> 1) + j;
        if (bz < 0 || bz >= (int64_t)ns) continue;
        const uint32_t v = row[bz] >> sh;
        bits |= ((v & 1u) | ((v >> 3) & 2u)) << (2 * j);
    }
    return bits;
}

// dst voxel p in the box [lo, hi) takes (op) src voxel p + off.  One thread per destination WORD of the box's rows: it
// gathers the word's 4 columns x 8 z-neighbours from the up to 2 x 2 x 5 source bricks that hold them, whatever the
// offset's parity on any axis, and writes the word once -- a partly covered word is a masked read-modify-write, which
// needs no atomic because a word has one owner within a call.  Volumes of 4^3 (two rows to a word) are the exception:
// there a word's rows take atomics.
__global__ void k_copy_region(uint32_t* __restrict__ dst, uint32_t Sd, const uint8_t* __restrict__ src, uint32_t Ss,
                              uint32_t lx, uint32_t ly, uint32_t lz, uint32_t hx, uint32_t hy, uint32_t hz,
                              int64_t ox, int64_t oy, int64_t oz, int op)
{
    const uint32_t lo[3] = {lx, ly, lz}, hi[3] = {hx, hy, hz};
    const uint32_t n = Sd >> 1, ns = Ss >> 1;
    const BoxWords b = box_words(lo, hi);
    for (uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < b.items; it += (uint64_t)gridDim.x * blockDim.x) {
        RowWord r;
        if (!row_word(b, n, it, r)) continue;
        const uint32_t mask = box_mask(b, r);
        if (!mask) continue;
        // z of the word's first voxel, relative to the row (negative where the word starts in the row before: n = 2)
        const int64_t z0 = 2 * ((int64_t)(4u * r.w) - (int64_t)r.base);
        const int64_t sz = z0 + oz;
        const uint32_t odd = (uint32_t)(sz & 1);
        uint32_t bits = 0u;
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t col = (source_column(src, ns, 2 * (int64_t)r.cx + (k & 1u) + ox, 2 * (int64_t)r.cy + (k >> 1) + oy, sz - odd) >> odd) & 0xffu;
            // column bit z -> word bit (z >> 1) * 8 + (z & 1) * 4 + k
            for (uint32_t z = 0; z < 8u; ++z) bits |= ((col >> z) & 1u) << ((z >> 1) * 8u + (z & 1u) * 4u + k);
        }
        bits &= mask;
        store_box_word(dst, r.w, mask, bits, op, n < 4u);
    }
}

// ---- queries -------------------------------------------------------------------

__global__ void k_get_voxels(const uint8_t* __restrict__ bricks, uint32_t S, uint64_t count, const uint32_t* __restrict__ xyz, uint8_t* __restrict__ solid_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    uint32_t v = 0u;
    if (x < S && y < S && z < S) v = (bricks[brick_of(S >> 1, x, y, z)] >> voxel_bit(x, y, z)) & 1u;
    solid_out[i] = (uint8_t)v;
}

// counts[box] (zeroed before the launch) += the solid voxels inside box: popcount of the words under k_fill_boxes' masks
__global__ void k_count_boxes(const uint32_t* __restrict__ words, uint32_t S, const uint32_t* __restrict__ lo_hi, unsigned long long* __restrict__ counts)
{
    __shared__ uint32_t part[4];
    uint32_t lo[3], hi[3];
    if (!clip_box(lo_hi + 6ull * blockIdx.x, S, lo, hi)) return;      // uniform for the workgroup
    const uint32_t n = S >> 1;
    const BoxWords b = box_words(lo, hi);
    uint32_t total = 0u;               // the largest box is 2^25 words: 2^22 voxels per thread, 2^30 per workgroup
    for (uint64_t it = (uint64_t)blockIdx.y * blockDim.x + threadIdx.x; it < b.items; it += (uint64_t)gridDim.y * blockDim.x) {
        RowWord r;
        if (!row_word(b, n, it, r)) continue;
        const uint32_t mask = box_mask(b, r);
        if (mask) total += __popc(words[r.w] & mask);
    }
    const uint32_t sum = group_sum<4u>(total, part);
    if (threadIdx.x == 0 && sum) atomicAdd(&counts[blockIdx.x], (unsigned long long)sum);
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
    __shared__ uint32_t part[4];
    uint32_t c = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * blockDim.x)
        c += __popc(words[i]);
    const uint32_t sum = group_sum<4u>(c, part);
    if (threadIdx.x == 0 && sum) atomicAdd(total, (unsigned long long)sum);
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
    if (v->d_flood) (void)hipFree(v->d_flood);
    if (v->d_marks) (void)hipFree(v->d_marks);
    if (v->d_surface) (void)hipFree(v->d_surface);
    if (v->d_rects) (void)hipFree(v->d_rects);
    if (v->d_pack) (void)hipFree(v->d_pack);
    if (v->d_levels) (void)hipFree(v->d_levels);
    if (v->d_morph) (void)hipFree(v->d_morph);
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

// workgroups per item for the kernels that take one item per blockIdx.x: a few items are spread over up to 1024
// workgroups each (a whole 1024^3 volume is 2^25 words); many items: one workgroup each.  A workgroup that finds
// nothing to do leaves at once.
uint32_t split_for(const vrc_volume* v, uint64_t n)
{
    uint32_t split = (uint32_t)((4096ull + n - 1) / n);
    const uint64_t max_words = v->n_bricks / 4u;
    const uint32_t useful = (uint32_t)((max_words + 255u) / 256u);   // 256-thread groups that cover the largest possible box once
    if (split > 1024u) split = 1024u;
    if (split > useful) split = useful;
    if (split == 0) split = 1;
    return split;
}

// max_radius: the largest radius of the batch where the caller knows it, -1 where it does not
void launch_fill_spheres(vrc_volume* v, uint64_t n, const int32_t* d_spheres, int32_t max_radius, int solid, hipStream_t st)
{
    // many small spheres (a brush at every hit of a batch: at most 6 x 6 x 3 words each): a wave each, not four
    const bool small = n >= 4096u && max_radius >= 0 && max_radius <= 4;
    hipLaunchKernelGGL(k_fill_spheres, dim3((uint32_t)n, split_for(v, n)), dim3(small ? 64 : 256), 0, st, v->d_bricks, 1u << v->depth,
                       d_spheres, solid ? 1u : 0u);
}

// The frame of the two brushes at hits: the n centres (x, y, z, radius) go into v's staging block, then fill(d_centres) enqueues
// the brush's own kernel.  Not a staged_call: the centres, no list of the caller's, go through the staging block in BOTH memory
// kinds (n x 4 int32, then the hits themselves when they come from the host), which an earlier call on another stream may still
// be reading -- so the call orders itself behind the volume's last edit and ends as an edit by hand.
template <class Fill>
int hits_call(const char* what, vrc_volume* v, uint64_t n, const vrc_hit* hits, int32_t radius, int solid, int mem, hipStream_t st, Fill fill)
{
    hipError_t e = hipSetDevice(v->device);
    if (e == hipSuccess) e = order_behind_edits(v, st);
    if (e == hipSuccess) e = reserve(v->d_stage, v->stage_cap, (size_t)n * (mem == VRC_MEM_HOST ? 64u : 16u));
    int32_t* d_centres = (int32_t*)v->d_stage;
    const vrc_hit* d_hits = hits;
    if (e == hipSuccess && mem == VRC_MEM_HOST) {
        d_hits = (const vrc_hit*)((uint8_t*)v->d_stage + (size_t)n * 16u);
        e = hipMemcpyAsync((void*)d_hits, hits, (size_t)n * sizeof(vrc_hit), hipMemcpyHostToDevice, st);
    }
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    hipLaunchKernelGGL(k_hits_to_centres, grid_for(n), dim3(256), 0, st, n, d_hits, v->depth, radius, solid ? 1u : 0u, d_centres);
    fill(d_centres);
    if ((e = hipGetLastError()) == hipSuccess) e = finish(v, mem, st, true);
    return done(e, what);
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
    const char* what = "vrc_volume_set_voxels";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (n == 0) return VRC_OK;
    if (!xyz) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, LANE_ITEMS, "voxels")) return rc;
    const Call call = edit_call(v, mem, stream);
    const StagePart parts[] = {{xyz, (size_t)n * 12u, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        hipLaunchKernelGGL(k_set_voxels, grid_for(n), dim3(256), 0, call.st, v->d_bricks, 1u << v->depth, n, (const uint32_t*)d[0], solid ? 1u : 0u);
        return hipSuccess;
    });
}

extern "C" int vrc_volume_fill_boxes(vrc_volume* v, uint64_t n, const uint32_t* lo_hi, int solid, int mem, void* stream)
{
    const char* what = "vrc_volume_fill_boxes";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (n == 0) return VRC_OK;
    if (!lo_hi) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, GROUP_ITEMS, "boxes")) return rc;
    const Call call = edit_call(v, mem, stream);
    const StagePart parts[] = {{lo_hi, (size_t)n * 24u, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        hipLaunchKernelGGL(k_fill_boxes, dim3((uint32_t)n, split_for(v, n)), dim3(256), 0, call.st, v->d_bricks, 1u << v->depth, (const uint32_t*)d[0],
                           solid ? 1u : 0u);
        return hipSuccess;
    });
}

extern "C" int vrc_volume_fill_spheres(vrc_volume* v, uint64_t n, const int32_t* centre_radius, int solid, int mem, void* stream)
{
    const char* what = "vrc_volume_fill_spheres";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (n == 0) return VRC_OK;
    if (!centre_radius) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, GROUP_ITEMS, "spheres")) return rc;
    const Call call = edit_call(v, mem, stream);
    const StagePart parts[] = {{centre_radius, (size_t)n * 16u, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        launch_fill_spheres(v, n, (const int32_t*)d[0], -1, solid, call.st);
        return hipSuccess;
    });
}

extern "C" int vrc_volume_fill_spheres_at_hits(vrc_volume* v, uint64_t n, const vrc_hit* hits, int32_t radius, int solid, int mem, void* stream)
{
    const char* what = "vrc_volume_fill_spheres_at_hits";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (radius < 0 || radius > VRC_BRUSH_LIMIT) return vrc::fail(VRC_ERR_INVALID, "%s: radius %d not in [0, 2^20]", what, radius);
    if (n == 0) return VRC_OK;
    if (!hits) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, GROUP_ITEMS, "hits")) return rc;
    hipStream_t st = (hipStream_t)stream;
    return hits_call(what, v, n, hits, radius, solid, mem, st, [&](const int32_t* d_centres) { launch_fill_spheres(v, n, d_centres, radius, solid, st); });
}

// ---- capsules (kernels: vrc_stroke.hip) ----------------------------------------------------------------------------

extern "C" int vrc_stroke_fill_capsules(vrc_volume* v, uint64_t n, const int32_t* items, int solid, int mem, void* stream)
{
    const char* what = "vrc_stroke_fill_capsules";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (n == 0) return VRC_OK;
    if (!items) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, GROUP_ITEMS, "capsules")) return rc;
    const Call call = edit_call(v, mem, stream);
    const StagePart parts[] = {{items, (size_t)n * 32u, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        vrc::stroke_capsules_run(v->d_bricks, v->depth, n, (const int32_t*)d[0], split_for(v, n), 256u, solid, call.st);
        return hipSuccess;
    });
}

extern "C" int vrc_stroke_fill_at_hits(vrc_volume* v, uint64_t n, const vrc_hit* hits, int32_t radius, uint32_t max_gap, int solid, int mem,
                                       void* stream)
{
    const char* what = "vrc_stroke_fill_at_hits";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (radius < 0 || radius > VRC_STROKE_LIMIT) return vrc::fail(VRC_ERR_INVALID, "%s: radius %d not in [0, 2^13]", what, radius);
    if (n == 0) return VRC_OK;
    if (!hits) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, GROUP_ITEMS, "hits")) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the links are read off neighbouring centres by the kernel, so the block holds no list of capsules; many thin strokes
    // between neighbouring hits: a wave each, as launch_fill_spheres
    return hits_call(what, v, n, hits, radius, solid, mem, st, [&](const int32_t* d_centres) {
        vrc::stroke_links_run(v->d_bricks, v->depth, n, d_centres, radius, max_gap, split_for(v, n), n >= 4096u && radius <= 4 ? 64u : 256u, solid, st);
    });
}

// ---- surface voxelisation (kernels: vrc_raster.hip) ------------------------------------------------------------------

extern "C" int vrc_raster_mesh(vrc_volume* v, uint64_t n, const int32_t* tris, int mode, int solid, int mem, void* stream)
{
    const char* what = "vrc_raster_mesh";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (mode != VRC_RASTER_TOUCHED && mode != VRC_RASTER_THIN) return vrc::fail(VRC_ERR_INVALID, "%s: unknown mode %d", what, mode);
    if (n == 0) return VRC_OK;
    if (!tris) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, GROUP_ITEMS, "triangles")) return rc;
    const Call call = edit_call(v, mem, stream);
    const StagePart parts[] = {{tris, (size_t)n * 36u, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        vrc::raster_run(v->d_bricks, v->depth, n, (const int32_t*)d[0], mode, solid, call.st);
        return hipSuccess;
    });
}

extern "C" int vrc_volume_xor_mesh(vrc_volume* v, uint64_t n, const int32_t* tris, int mem, void* stream)
{
    const char* what = "vrc_volume_xor_mesh";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (n == 0) return VRC_OK;
    if (!tris) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, GROUP_ITEMS, "triangles")) return rc;
    // the mark field is shared by every call and the scan's read-modify-write of the occupancy is not atomic: behind the
    // last asynchronous edit whatever the memory kind
    const Call call = shared_edit_call(v, mem, stream);
    const StagePart parts[] = {{tris, (size_t)n * 36u, STAGE_IN}};
    return staged_call(what, call, parts, [&](void* const* d) {
        hipError_t e = hipSuccess;
        if (!v->d_marks) {
            const size_t bytes = vrc::voxelize_scratch_bytes(v->depth);
            if ((e = hipMalloc((void**)&v->d_marks, bytes)) == hipSuccess) e = hipMemsetAsync(v->d_marks, 0, bytes, call.st);
            if (e != hipSuccess && v->d_marks) { (void)hipFree(v->d_marks); v->d_marks = nullptr; }
        }
        if (e == hipSuccess) vrc::voxelize_run(v->d_bricks, v->d_marks, v->depth, n, (const int32_t*)d[0], call.st);
        return e;
    });
}

extern "C" int vrc_volume_copy_region(vrc_volume* dst, vrc_volume* src, const uint32_t src_lo[3], const uint32_t size[3], const int32_t dst_lo[3],
                                      int op, void* stream)
{
    const char* what = "vrc_volume_copy_region";
    if (!dst || !src || !src_lo || !size || !dst_lo) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_distinct(what, src, dst)) return rc;      // ahead of the op, the devices behind it: the order the refusals always had
    if (const int rc = check_op(what, op)) return rc;
    if (const int rc = check_pair(what, src, dst, false)) return rc;
    // the region clipped to both volumes, as the destination's voxel box [lo, hi) and the offset to the source
    const int64_t Ss = 1ll << src->depth, Sd = 1ll << dst->depth;
    uint32_t lo[3], hi[3];
    int64_t off[3];
    for (int a = 0; a < 3; ++a) {
        int64_t d0 = 0, d1 = size[a];                                  // 0 <= d0 <= d < d1 <= size
        if (-(int64_t)dst_lo[a] > d0) d0 = -(int64_t)dst_lo[a];
        if (Ss - (int64_t)src_lo[a] < d1) d1 = Ss - (int64_t)src_lo[a];
        if (Sd - (int64_t)dst_lo[a] < d1) d1 = Sd - (int64_t)dst_lo[a];
        if (d0 >= d1) return VRC_OK;                                   // nothing of the region lies in both volumes
        lo[a] = (uint32_t)(dst_lo[a] + d0);
        hi[a] = (uint32_t)(dst_lo[a] + d1);
        off[a] = (int64_t)src_lo[a] - (int64_t)dst_lo[a];
    }
    const Call call = pair_call(dst, src, VRC_MEM_DEVICE, stream);
    return staged_call(what, call, [&]() {
        hipLaunchKernelGGL(k_copy_region, dim3(box_launch_groups(lo, hi)), dim3(256), 0, call.st, dst->d_bricks, (uint32_t)Sd, (const uint8_t*)src->d_bricks,
                           (uint32_t)Ss, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], off[0], off[1], off[2], op);
        return hipSuccess;
    });
}

extern "C" int vrc_volume_stamp_affine(vrc_volume* dst, vrc_volume* src, const vrc_affine* map, const uint32_t dst_lo[3], const uint32_t dst_hi[3],
                                       int op, void* stream)
{
    const char* what = "vrc_volume_stamp_affine";
    if (!dst || !src || !map || !dst_lo || !dst_hi) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_distinct(what, src, dst)) return rc;      // as vrc_volume_copy_region
    if (const int rc = check_op(what, op)) return rc;
    if (const int rc = check_affine(what, map, -1)) return rc;
    if (const int rc = check_pair(what, src, dst, false)) return rc;
    const uint32_t box[6] = {dst_lo[0], dst_lo[1], dst_lo[2], dst_hi[0], dst_hi[1], dst_hi[2]};
    uint32_t lo[3], hi[3];
    if (!clip_box(box, 1u << dst->depth, lo, hi)) return VRC_OK;       // empty, inverted or wholly outside: nothing to write
    const Call call = pair_call(dst, src, VRC_MEM_DEVICE, stream);
    return staged_call(what, call, [&]() {
        vrc::stamp_affine_run(dst->d_bricks, dst->depth, src->d_bricks, src->depth, *map, lo, hi, op, call.st);
        return hipSuccess;
    });
}

extern "C" int vrc_volume_clone(vrc_volume* src, vrc_volume** out)
{
    if (!src || !out) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_clone: null argument");
    vrc_volume* v = nullptr;
    int rc = volume_new(src->depth, src->device, &v);
    if (rc) return rc;
    rc = staged_call("vrc_volume_clone", null_stream_call(src, nullptr, false, true), [&]() {
        const hipError_t e = hipMemcpyAsync(v->d_bricks, src->d_bricks, src->n_bricks, hipMemcpyDeviceToDevice, nullptr);
        return e != hipSuccess ? e : hipMemcpyAsync(v->d_tex, src->d_tex, 1536, hipMemcpyDeviceToDevice, nullptr);
    });
    if (rc) { volume_free(v); return rc; }
    *out = v;
    return VRC_OK;
}

extern "C" int vrc_volume_get_voxels(vrc_volume* v, uint64_t n, const uint32_t* xyz, uint8_t* solid_out, int mem, void* stream)
{
    const char* what = "vrc_volume_get_voxels";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (n == 0) return VRC_OK;
    if (!xyz || !solid_out) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, LANE_ITEMS, "voxels")) return rc;
    const Call call = query_call(v, mem, stream);
    const StagePart parts[] = {{xyz, (size_t)n * 12u, STAGE_IN}, {solid_out, (size_t)n, STAGE_OUT}};
    return staged_call(what, call, parts, [&](void* const* d) {
        hipLaunchKernelGGL(k_get_voxels, grid_for(n), dim3(256), 0, call.st, (const uint8_t*)v->d_bricks, 1u << v->depth, n, (const uint32_t*)d[0], (uint8_t*)d[1]);
        return hipSuccess;
    });
}

extern "C" int vrc_volume_count_boxes(vrc_volume* v, uint64_t n, const uint32_t* lo_hi, uint64_t* counts, int mem, void* stream)
{
    const char* what = "vrc_volume_count_boxes";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (n == 0) return VRC_OK;
    if (!lo_hi || !counts) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer", what);
    if (const int rc = check_count(what, n, GROUP_ITEMS, "boxes")) return rc;
    const Call call = query_call(v, mem, stream);
    const StagePart parts[] = {{lo_hi, (size_t)n * 24u, STAGE_IN}, {counts, (size_t)n * 8u, STAGE_OUT}};
    return staged_call(what, call, parts, [&](void* const* d) {
        const hipError_t e = hipMemsetAsync(d[1], 0, (size_t)n * 8u, call.st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_count_boxes, dim3((uint32_t)n, split_for(v, n)), dim3(256), 0, call.st, v->d_bricks, 1u << v->depth, (const uint32_t*)d[0],
                           (unsigned long long*)d[1]);
        return hipSuccess;
    });
}

// ---- the two meshes: exposed faces (vrc_surface.hip) and merged rectangles (vrc_rects.hip) -------------------------

// What the two extractors differ in.  Each keeps a block of its own in the volume (offsets, totals; the rectangles' row
// fields), allocated by the first call and fixed in size.
struct MeshRuns {
    hipError_t (*reserve)(vrc_volume* v);
    void (*prepare)(vrc_volume* v, hipStream_t st);                 // what every later pass reads; nullptr: nothing
    void (*count)(vrc_volume* v, int closed, hipStream_t st);
    void (*offsets)(vrc_volume* v, int closed, unsigned long long* d_total, hipStream_t st);
    void (*emit)(vrc_volume* v, int closed, int format, uint64_t first, uint64_t n, void* out, hipStream_t st);
    unsigned long long* (*total_slot)(vrc_volume* v);
    unsigned long long* (*direction_slots)(vrc_volume* v);
};

const MeshRuns SURFACE = {
    [](vrc_volume* v) { return v->d_surface ? hipSuccess : hipMalloc((void**)&v->d_surface, vrc::surface_scratch_bytes(v->depth)); },
    nullptr,
    [](vrc_volume* v, int closed, hipStream_t st) { vrc::surface_count_run(v->d_bricks, v->depth, closed, v->d_surface, st); },
    [](vrc_volume* v, int closed, unsigned long long* d_total, hipStream_t st) { vrc::surface_offsets_run(v->d_bricks, v->depth, closed, v->d_surface, d_total, st); },
    [](vrc_volume* v, int closed, int format, uint64_t first, uint64_t n, void* out, hipStream_t st) {
        vrc::surface_emit_run(v->d_bricks, v->depth, closed, format, first, n, out, v->d_surface, st);
    },
    [](vrc_volume* v) { return vrc::surface_total_slot(v->d_surface, v->depth); },
    [](vrc_volume* v) { return vrc::surface_direction_slots(v->d_surface, v->depth); },
};

const MeshRuns RECTS = {
    [](vrc_volume* v) { return v->d_rects ? hipSuccess : hipMalloc((void**)&v->d_rects, vrc::rect_scratch_bytes(v->depth)); },
    [](vrc_volume* v, hipStream_t st) { vrc::rect_rows_run(v->d_bricks, v->depth, v->d_rects, st); },
    [](vrc_volume* v, int closed, hipStream_t st) { vrc::rect_count_run(v->depth, closed, v->d_rects, st); },
    [](vrc_volume* v, int closed, unsigned long long* d_total, hipStream_t st) { vrc::rect_offsets_run(v->depth, closed, v->d_rects, d_total, st); },
    [](vrc_volume* v, int closed, int format, uint64_t first, uint64_t n, void* out, hipStream_t st) {
        vrc::rect_emit_run(v->depth, closed, format, first, n, out, v->d_rects, st);
    },
    [](vrc_volume* v) { return vrc::rect_total_slot(v->d_rects, v->depth); },
    [](vrc_volume* v) { return vrc::rect_direction_slots(v->d_rects, v->depth); },
};

// the per-direction totals: synchronous on the NULL stream, behind the last asynchronous edit (a device-memory extraction,
// which shares the block, included)
static int mesh_count(const char* what, const MeshRuns& runs, vrc_volume* v, int closed, uint64_t counts[6])
{
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (!counts) return vrc::fail(VRC_ERR_INVALID, "%s: null counts", what);
    unsigned long long host[6];
    const int rc = staged_call(what, null_stream_call(v, nullptr, false, false), [&]() {
        hipError_t e = runs.reserve(v);
        if (e != hipSuccess) return e;
        if (runs.prepare) runs.prepare(v, nullptr);
        runs.count(v, closed, nullptr);
        if ((e = hipGetLastError()) == hipSuccess) e = hipMemcpy(host, runs.direction_slots(v), sizeof host, hipMemcpyDeviceToHost);
        return e;
    });
    for (int d = 0; d < 6 && !rc; ++d) counts[d] = host[d];
    return rc;
}

// Records [first, first + capacity) of a list in its canonical order, and its total: the frame of the face, rectangle and
// voxel extractions, after their argument checks.  reserve(): the extractor's block; offsets(d_total, st): passes 1 and 2;
// emit(first, n, out, st): pass 3; total_slot(): where pass 2 leaves the total.  Device memory: asynchronous on the caller's
// stream.  Host memory: synchronous; the total is read back first, then the records come through the volume's staging
// block in windows of at most 2^20.
template <class Reserve, class Offsets, class Emit, class TotalSlot>
static int windowed_extract(const char* what, vrc_volume* v, size_t record, uint64_t first, uint64_t capacity, void* out, uint64_t* total, int mem,
                            hipStream_t st, Reserve reserve_block, Offsets offsets, Emit emit, TotalSlot total_slot)
{
    // behind the last asynchronous edit whatever the memory kind: the extractor's block is shared by every call.  Not a
    // staged_call: the host form reads the total back before it knows its windows, and synchronises between them
    hipError_t e = hipSetDevice(v->device);
    if (e == hipSuccess) e = order_behind_edits(v, st);
    if (e == hipSuccess) e = reserve_block();
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    if (mem == VRC_MEM_DEVICE) {
        offsets((unsigned long long*)total, st);
        if (capacity) emit(first, capacity, out, st);
        // recorded as an edit: the next call, on whatever stream, must not rewrite the block under this one
        if ((e = hipGetLastError()) == hipSuccess) e = finish(v, mem, st, true);
        return done(e, what);
    }
    offsets(nullptr, st);
    e = hipGetLastError();
    unsigned long long T = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&T, total_slot(), 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    if (total) *total = T;
    // the block stays valid for every window: the call holds the stream until it returns
    const uint64_t want = window_of(first, capacity, T);
    const uint64_t window = want < (1ull << 20) ? want : (1ull << 20);
    if (want) e = reserve(v->d_stage, v->stage_cap, (size_t)window * record);
    for (uint64_t at = 0; at < want && e == hipSuccess; at += window) {
        const uint64_t now = want - at < window ? want - at : window;
        emit(first + at, now, v->d_stage, st);
        if ((e = hipGetLastError()) == hipSuccess) e = hipMemcpyAsync((uint8_t*)out + at * record, v->d_stage, (size_t)now * record, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = finish(v, mem, st, false);
    return done(e, what);
}

// the checks every windowed extraction shares: the memory kind, a buffer for the capacity, a device buffer's alignment
static int check_window(const char* what, uint64_t capacity, const void* out, int mem, unsigned align)
{
    if (const int rc = check_mem(what, mem)) return rc;
    if (!out && capacity) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer with capacity %llu", what, (unsigned long long)capacity);
    if (mem == VRC_MEM_DEVICE && capacity && ((uintptr_t)out & (align - 1u)))
        return vrc::fail(VRC_ERR_INVALID, "%s: device buffer %p is not aligned to %u bytes", what, out, align);
    return VRC_OK;
}

static int mesh_extract(const char* what, const MeshRuns& runs, vrc_volume* v, int closed, int format, uint64_t first, uint64_t capacity, void* out,
                        uint64_t* total, int mem, void* stream)
{
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (format != VRC_SURFACE_FACES && format != VRC_SURFACE_TRIANGLES) return vrc::fail(VRC_ERR_INVALID, "%s: bad format %d", what, format);
    if (const int rc = check_window(what, capacity, out, mem, format == VRC_SURFACE_FACES ? 16u : 4u)) return rc;
    return windowed_extract(
        what, v, format == VRC_SURFACE_FACES ? 16u : 72u, first, capacity, out, total, mem, (hipStream_t)stream, [&]() { return runs.reserve(v); },
        [&](unsigned long long* d_total, hipStream_t st) {
            if (runs.prepare) runs.prepare(v, st);
            runs.offsets(v, closed, d_total, st);
        },
        [&](uint64_t at, uint64_t n, void* to, hipStream_t st) { runs.emit(v, closed, format, at, n, to, st); }, [&]() { return runs.total_slot(v); });
}

// ---- the voxel lists (kernels: vrc_voxels.hip) ----------------------------------------------------------------------

// `which`, and the box clipped to the volume (NULL: the whole of it); an empty box selects nothing
static int voxel_query(const char* what, const vrc_volume* v, int which, int closed, const uint32_t* lo_hi, vrc::VoxelQuery* q)
{
    if (which != VRC_VOXELS_ALL && which != VRC_VOXELS_SURFACE && which != VRC_VOXELS_INTERIOR) return vrc::fail(VRC_ERR_INVALID, "%s: bad which %d", what, which);
    const uint32_t S = 1u << v->depth, whole[6] = {0u, 0u, 0u, S, S, S};
    if (!clip_box(lo_hi ? lo_hi : whole, S, q->lo, q->hi))
        for (int a = 0; a < 3; ++a) q->lo[a] = q->hi[a] = 0u;
    q->which = which;
    q->closed = closed;
    return VRC_OK;
}

// the lists share the surface calls' offsets block: the same slots, of which they use all but the six direction totals
static hipError_t reserve_voxel_slots(vrc_volume* v)
{
    return v->d_surface ? hipSuccess : hipMalloc((void**)&v->d_surface, vrc::surface_scratch_bytes(v->depth));
}

extern "C" int vrc_voxels_count(vrc_volume* v, int which, int closed, const uint32_t* lo_hi, uint64_t* count)
{
    const char* what = "vrc_voxels_count";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (!count) return vrc::fail(VRC_ERR_INVALID, "%s: null count", what);
    vrc::VoxelQuery q;
    if (const int rc = voxel_query(what, v, which, closed, lo_hi, &q)) return rc;
    // synchronous on the NULL stream, behind the last asynchronous edit (a device-memory extraction, which shares the
    // block, included)
    unsigned long long T = 0;
    const int rc = staged_call(what, null_stream_call(v, nullptr, false, false), [&]() {
        hipError_t e = reserve_voxel_slots(v);
        if (e != hipSuccess) return e;
        vrc::voxels_offsets_run(v->d_bricks, v->depth, q, v->d_surface, nullptr, nullptr);
        if ((e = hipGetLastError()) == hipSuccess) e = hipMemcpy(&T, vrc::voxels_total_slot(v->d_surface, v->depth), 8, hipMemcpyDeviceToHost);
        return e;
    });
    if (!rc) *count = T;
    return rc;
}

extern "C" int vrc_voxels_extract(vrc_volume* v, int which, int closed, const uint32_t* lo_hi, int format, uint64_t first, uint64_t capacity, void* out,
                                  uint64_t* total, int mem, void* stream)
{
    const char* what = "vrc_voxels_extract";
    if (!v) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    vrc::VoxelQuery q;
    if (const int rc = voxel_query(what, v, which, closed, lo_hi, &q)) return rc;
    if (format != VRC_VOXELS_XYZ && format != VRC_VOXELS_NEIGHBOURS) return vrc::fail(VRC_ERR_INVALID, "%s: bad format %d", what, format);
    if (const int rc = check_window(what, capacity, out, mem, format == VRC_VOXELS_XYZ ? 4u : 16u)) return rc;
    return windowed_extract(
        what, v, format == VRC_VOXELS_XYZ ? 12u : 16u, first, capacity, out, total, mem, (hipStream_t)stream, [&]() { return reserve_voxel_slots(v); },
        [&](unsigned long long* d_total, hipStream_t st) { vrc::voxels_offsets_run(v->d_bricks, v->depth, q, v->d_surface, d_total, st); },
        [&](uint64_t at, uint64_t n, void* to, hipStream_t st) { vrc::voxels_emit_run(v->d_bricks, v->depth, q, format, at, n, to, v->d_surface, st); },
        [&]() { return vrc::voxels_total_slot(v->d_surface, v->depth); });
}

extern "C" int vrc_volume_surface_count(vrc_volume* v, int closed, uint64_t counts[6])
{
    return mesh_count("vrc_volume_surface_count", SURFACE, v, closed, counts);
}

extern "C" int vrc_volume_extract_surface(vrc_volume* v, int closed, int format, uint64_t first, uint64_t capacity, void* out, uint64_t* total,
                                          int mem, void* stream)
{
    return mesh_extract("vrc_volume_extract_surface", SURFACE, v, closed, format, first, capacity, out, total, mem, stream);
}

extern "C" int vrc_rect_count(vrc_volume* v, int closed, uint64_t counts[6])
{
    return mesh_count("vrc_rect_count", RECTS, v, closed, counts);
}

extern "C" int vrc_extract_rects(vrc_volume* v, int closed, int format, uint64_t first, uint64_t capacity, void* out, uint64_t* total, int mem,
                                        void* stream)
{
    return mesh_extract("vrc_extract_rects", RECTS, v, closed, format, first, capacity, out, total, mem, stream);
}

extern "C" int vrc_volume_flood(vrc_volume* region, vrc_volume* medium, int connectivity, int through, uint32_t max_sweeps, vrc_flood_stats* stats)
{
    const char* what = "vrc_volume_flood";
    if (!region || !medium) return vrc::fail(VRC_ERR_INVALID, "%s: null volume", what);
    if (region == medium) return vrc::fail(VRC_ERR_INVALID, "%s: region and medium are the same volume", what);
    if (const int rc = check_connectivity(what, connectivity)) return rc;
    if (const int rc = check_through(what, through)) return rc;
    if (const int rc = check_pair(what, region, medium, true)) return rc;
    // the NULL stream, behind the last asynchronous edit of either volume, as commit / download are; recorded as region's last
    // edit: edits on streams made by vrc_stream_create do not wait for the NULL stream
    uint32_t sweeps = 0, converged = 0;
    const int flooded = staged_call(what, null_stream_call(region, medium, true, false), [&]() {
        const hipError_t e = reserve(region->d_flood, region->flood_cap, vrc::flood_scratch_bytes(region->depth));
        return e != hipSuccess ? e : vrc::flood_run(region->d_bricks, medium->d_bricks, region->depth, connectivity, through,
                                                    max_sweeps ? max_sweeps : vrc::flood_sweep_bound(region->depth), region->d_flood, nullptr, &sweeps, &converged);
    });
    if (flooded) return flooded;
    if (stats) {
        uint64_t reached = 0;
        const int rc = vrc_volume_solid_count(region, &reached);
        if (rc) return rc;
        stats->reached = reached; stats->sweeps = sweeps; stats->converged = converged;
    }
    return VRC_OK;
}

extern "C" int vrc_volume_commit(vrc_volume* v, vrc_scene** out, float* build_ms)
{
    if (!v || !out) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_commit: null argument");
    // not a staged_call: the builder is a frame of its own, with its own texts, timing and synchronisation; only the wait is the volume's
    hipError_t e = hipSetDevice(v->device);
    if (e == hipSuccess) e = order_behind_edits(v, nullptr);
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
    // the dense bytes are the call's one list, in host memory: staged in a block of the call's own, on the NULL stream
    const uint64_t S = 1ull << v->depth;
    const StagePart parts[] = {{solid_host, (size_t)(S * S * S), STAGE_OUT}};
    return staged_call("vrc_volume_download", volume_call(v->device, VRC_MEM_HOST, nullptr, v, false), parts, [&](void* const* d) {
        hipLaunchKernelGGL(k_expand_dense, grid_for(S * S * S / 4u), dim3(256), 0, nullptr, (const uint8_t*)v->d_bricks, (uint32_t)S, (uint32_t*)d[0]);
        return hipSuccess;
    });
}

extern "C" int vrc_volume_edit_scratch_bytes(const vrc_volume* v, uint64_t* bytes)
{
    if (!v || !bytes) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_edit_scratch_bytes: null argument");
    *bytes = (uint64_t)v->stage_cap + (uint64_t)v->flood_cap + (v->d_marks ? (uint64_t)vrc::voxelize_scratch_bytes(v->depth) : 0u) +
             (v->d_surface ? (uint64_t)vrc::surface_scratch_bytes(v->depth) : 0u) + (v->d_rects ? (uint64_t)vrc::rect_scratch_bytes(v->depth) : 0u) +
             (v->d_pack ? (uint64_t)vrc::pack_scratch_bytes(v->depth) : 0u);
    return VRC_OK;
}

extern "C" int vrc_volume_solid_count(vrc_volume* v, uint64_t* count)
{
    if (!v || !count) return vrc::fail(VRC_ERR_INVALID, "vrc_volume_solid_count: null argument");
    unsigned long long total = 0;
    const int rc = staged_call("vrc_volume_solid_count", null_stream_call(v, nullptr, false, false), [&]() {
        hipError_t e = hipMemsetAsync(v->d_count, 0, 8, nullptr);
        if (e != hipSuccess) return e;
        const uint64_t n_words = v->n_bricks / 4u;
        uint64_t groups = (n_words + 255u) / 256u;
        if (groups > 4096u) groups = 4096u;
        hipLaunchKernelGGL(k_count_solid, dim3((uint32_t)groups), dim3(256), 0, nullptr, v->d_bricks, n_words, v->d_count);
        if ((e = hipGetLastError()) == hipSuccess) e = hipMemcpy(&total, v->d_count, 8, hipMemcpyDeviceToHost);
        return e;
    });
    if (!rc) *count = total;
    return rc;
}

// ---- the sparse tile stream (vrc.h: vrc_pack_*; kernels and format arithmetic: vrc_pack.hip, vrc_pack.h) ------------

namespace {

// The header rules, in the order of include/vrc.h, over the 16 header words h (nullptr when bytes < 64): nullptr, or the
// name of the first rule that does not hold.  expect_depth == 0: any depth in 2..10 passes the depth rule.
const char* pack_header_rule(const uint32_t* h, uint64_t bytes, uint32_t expect_depth)
{
    if (bytes < vrc::PACK_HEADER_BYTES || !h) return "header-short";
    if (h[0] != vrc::PACK_MAGIC || h[1] != vrc::PACK_VERSION) return "magic-version";
    const uint32_t depth = h[2];
    if (depth < 2u || depth > 10u || (expect_depth && depth != expect_depth)) return "depth";
    const uint32_t nt = vrc::pack_tiles(depth), M = h[4], P = h[5], full = h[10];
    if (h[3] != nt) return "tiles";
    for (int k = 11; k < 16; ++k)
        if (h[k]) return "reserved";
    const uint64_t length = (uint64_t)h[6] | ((uint64_t)h[7] << 32);
    if (length != bytes) return "length-argument";
    if (length != vrc::pack_layout(depth, M, P).length) return "length-formula";
    if (M > nt || (uint64_t)P > (uint64_t)vrc::pack_tile_bricks(depth) * M || (uint64_t)full + M > nt) return "count-limits";
    return nullptr;
}

void pack_info_of(const uint32_t* h, vrc_pack_info* info)
{
    info->depth = h[2]; info->tiles = h[3]; info->mixed_tiles = h[4]; info->full_tiles = h[10]; info->partial_bricks = h[5]; info->reserved = 0;
    info->bytes = (uint64_t)h[6] | ((uint64_t)h[7] << 32);
    info->solid = (uint64_t)h[8] | ((uint64_t)h[9] << 32);
}

hipError_t pack_scratch(vrc_volume* v)
{
    return v->d_pack ? hipSuccess : hipMalloc(&v->d_pack, vrc::pack_scratch_bytes(v->depth));
}

}  // namespace

extern "C" uint64_t vrc_pack_bound(uint32_t depth) { return depth < 2u || depth > 10u ? 0u : vrc::pack_bound_bytes(depth); }

extern "C" int vrc_pack_header(const void* data, uint64_t bytes, vrc_pack_info* out)
{
    const char* what = "vrc_pack_header";
    if (!data || !out) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    uint32_t h[16];
    if (bytes >= vrc::PACK_HEADER_BYTES) memcpy(h, data, sizeof h);
    if (const char* rule = pack_header_rule(bytes >= vrc::PACK_HEADER_BYTES ? h : nullptr, bytes, 0u)) return vrc::fail(VRC_ERR_INVALID, "%s: rule %s", what, rule);
    pack_info_of(h, out);
    return VRC_OK;
}

extern "C" int vrc_pack_volume(vrc_volume* v, void* out, uint64_t capacity, vrc_pack_info* info, int mem)
{
    const char* what = "vrc_pack_volume";
    if (!v || !info) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (!out && capacity) return vrc::fail(VRC_ERR_INVALID, "%s: null buffer with capacity %llu", what, (unsigned long long)capacity);
    if (out && mem == VRC_MEM_DEVICE && ((uintptr_t)out & 3u)) return vrc::fail(VRC_ERR_INVALID, "%s: device buffer %p is not aligned to 4 bytes", what, out);
    // not a staged_call: the host reads the totals back, sizes and refuses by them, and only then emits
    hipError_t e = hipSetDevice(v->device);
    if (e == hipSuccess) e = order_behind_edits(v, nullptr);
    if (e == hipSuccess) e = pack_scratch(v);
    vrc::PackTotals totals;
    if (e == hipSuccess) {
        vrc::pack_offsets_run(v->d_bricks, v->depth, v->d_pack, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(&totals, v->d_pack, sizeof totals, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    const uint64_t bytes = vrc::pack_layout(v->depth, totals.mixed, totals.partial).length;
    info->depth = v->depth; info->tiles = vrc::pack_tiles(v->depth); info->mixed_tiles = totals.mixed; info->full_tiles = totals.full;
    info->partial_bricks = totals.partial; info->reserved = 0; info->bytes = bytes; info->solid = totals.solid;
    if (!out) return VRC_OK;
    if (capacity < bytes)
        return vrc::fail(VRC_ERR_INVALID, "%s: capacity %llu below the stream's %llu bytes", what, (unsigned long long)capacity, (unsigned long long)bytes);
    uint8_t* own = nullptr;
    if (mem == VRC_MEM_HOST) e = hipMalloc((void**)&own, bytes);
    if (e == hipSuccess) {
        vrc::pack_emit_run(v->d_bricks, v->depth, v->d_pack, totals, own ? own : (uint8_t*)out, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = own ? hipMemcpy(out, own, bytes, hipMemcpyDeviceToHost) : hipStreamSynchronize(nullptr);
    if (own) (void)hipFree(own);
    return done(e, what);
}

extern "C" int vrc_unpack_volume(vrc_volume* v, const void* data, uint64_t bytes, int mem)
{
    const char* what = "vrc_unpack_volume";
    if (!v || !data) return vrc::fail(VRC_ERR_INVALID, "%s: null argument", what);
    if (const int rc = check_mem(what, mem)) return rc;
    if (mem == VRC_MEM_DEVICE && ((uintptr_t)data & 3u)) return vrc::fail(VRC_ERR_INVALID, "%s: device buffer %p is not aligned to 4 bytes", what, data);
    if (bytes < vrc::PACK_HEADER_BYTES) return vrc::fail(VRC_ERR_INVALID, "%s: rule %s", what, pack_header_rule(nullptr, bytes, v->depth));
    uint32_t h[16];
    hipError_t e = hipSuccess;
    if (mem == VRC_MEM_HOST) memcpy(h, data, sizeof h);
    else {
        e = hipSetDevice(v->device);
        if (e == hipSuccess) e = hipMemcpy(h, data, sizeof h, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return vrc::fail_hip(e, what);
    }
    if (const char* rule = pack_header_rule(h, bytes, v->depth)) return vrc::fail(VRC_ERR_INVALID, "%s: rule %s", what, rule);
    const uint32_t M = h[4], P = h[5];
    // not a staged_call: the host reads the check's findings back and writes only a stream that broke no rule
    e = hipSetDevice(v->device);
    if (e == hipSuccess) e = order_behind_edits(v, nullptr);
    if (e == hipSuccess) e = pack_scratch(v);
    uint8_t* own = nullptr;
    if (e == hipSuccess && mem == VRC_MEM_HOST) {
        e = hipMalloc((void**)&own, bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(own, data, bytes, hipMemcpyHostToDevice, nullptr);
    }
    const uint8_t* d = own ? own : (const uint8_t*)data;
    vrc::PackTotals t;
    if (e == hipSuccess) {
        vrc::unpack_check_run(d, v->depth, M, P, v->d_pack, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(&t, v->d_pack, sizeof t, hipMemcpyDeviceToHost);
    // the device-side rules in the order of include/vrc.h: the first that broke, with the least tile or byte where it has one
    const char* rule = nullptr;
    const char* unit = nullptr;
    uint32_t at = 0u;
    if (e == hipSuccess) {
        const uint64_t solid = t.solid + 8ull * vrc::pack_tile_bricks(v->depth) * t.full, claimed = (uint64_t)h[8] | ((uint64_t)h[9] << 32);
        const struct { const char* name; bool broken; const char* unit; uint32_t at; } rules[] = {
            {"class-map", t.first_class != ~0u, "tile", t.first_class},
            {"mixed-count", t.mixed != M, nullptr, 0u},
            {"full-count", t.full != h[10], nullptr, 0u},
            {"full-in-some", t.first_subset != ~0u, "tile", t.first_subset},
            {"mask-range", t.first_range != ~0u, "tile", t.first_range},
            {"some-empty", t.first_empty != ~0u, "tile", t.first_empty},
            {"full-whole", t.first_whole != ~0u, "tile", t.first_whole},
            {"partial-count", t.first_count != ~0u, "tile", t.first_count},
            {"partial-sum", t.partial != P, nullptr, 0u},
            {"partial-byte", t.first_byte != ~0u, "byte", t.first_byte},
            {"padding", t.first_padding != ~0u, "byte", t.first_padding},
            {"solid-count", solid != claimed, nullptr, 0u}};
        for (const auto& r : rules)
            if (r.broken) { rule = r.name; unit = r.unit; at = r.at; break; }
    }
    if (e == hipSuccess && !rule) {
        vrc::unpack_write_run(d, v->depth, M, P, v->d_pack, v->d_bricks, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    if (own) (void)hipFree(own);
    if (e != hipSuccess) return vrc::fail_hip(e, what);
    if (rule && unit) return vrc::fail(VRC_ERR_INVALID, "%s: rule %s at %s %u", what, rule, unit, at);
    if (rule) return vrc::fail(VRC_ERR_INVALID, "%s: rule %s", what, rule);
    return VRC_OK;
}
