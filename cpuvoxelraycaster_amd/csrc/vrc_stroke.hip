// vrc_stroke.hip -- the capsule brush (include/vrc.h: vrc_stroke_*; the rule, the pieces and the launches: vrc_stroke.h).
//
// blockIdx.x = capsule, its work split over blockIdx.y x blockDim.x threads, as the spheres of vrc_volume.hip.  A capsule is
// never walked by its bounding box -- a radius-3 diagonal of 512^3 has the whole volume as its box -- but piece by piece
// (stroke_piece_box): the work items of a capsule are the occupancy words (BoxWords) of its pieces' boxes, the capsule's
// workgroups are dealt out over the pieces, and within a piece a thread takes every stride-th word, adjacent lanes adjacent
// words of a brick row.  A piece box is computed from the capsule alone: uniform for the workgroup.
//
// A word is 2 x 2 columns of 8 voxels along z.  It is first held against the capsule as a whole: the centre of its voxels'
// box in doubled coordinates, with the radius grown by the box's half diagonal; most words of a thin capsule's piece boxes
// leave there.  Then each column walks its 8 voxels with q.q and t = q.d advanced by additions.  Inside a volume of at most
// 1024^3 and with items inside VRC_STROKE_LIMIT, q.q, L2 and |t| fit 32 bits (vrc.h), so the two products of a voxel,
// (q.q) L2 and t^2, are 32 x 32 -> 64 multiplies and not full 64-bit ones, which cost three of those and more.  The three
// cases of the rule are selected, not branched on: lanes of a wave sit in different cases at the two ends of a capsule.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vrc_box_words.h"
#include "vrc_stroke.h"

namespace {

// what a voxel is held against: the capsule with its derived constants
struct Rule {
    int32_t a[3], d[3];
    uint32_t L2;               // < 2^30
    int64_t r2, r2L2;          // r^2 <= 2^26, r^2 L2 < 2^56
};

// the rule of vrc.h for q = p - a given as q.q and t = q.d
__device__ __forceinline__ bool inside(const Rule& u, int32_t qq, int32_t t)
{
    const bool at_a = u.L2 == 0u || t <= 0, at_b = t >= 0 && (uint32_t)t >= u.L2;
    const int64_t side = (int64_t)((uint64_t)(uint32_t)qq * u.L2) - (int64_t)t * t;         // |p - line|^2 L2, both products < 2^58
    const int64_t cap = at_a ? qq : (int64_t)qq - 2 * (int64_t)t + (int64_t)u.L2;           // |p - a|^2 or |p - b|^2
    return (at_a || at_b) ? cap <= u.r2 : side <= u.r2L2;
}

// The same rule for a point given in doubled coordinates (Q = 2 q, T = Q.d) against the radius R / 2: the centre of a word's
// voxels.  Q.Q < 2^30, |T| < 2^30, R < 2^15: Q.Q L2 and T^2 < 2^60, R^2 L2 < 2^60.
__device__ __forceinline__ bool near(const Rule& u, int64_t QQ, int64_t T, int64_t R)
{
    const int64_t L2 = u.L2;
    if (L2 == 0 || T <= 0) return QQ <= R * R;
    if (T >= 2 * L2) return QQ - 4 * T + 4 * L2 <= R * R;
    return QQ * L2 - T * T <= R * R * L2;
}

__device__ __forceinline__ void fill_capsule(uint32_t* __restrict__ words, uint32_t S, const vrc::Capsule& c, uint32_t solid)
{
    const vrc::StrokePieces ps = vrc::stroke_pieces(c, S);
    if (!ps.count) return;                                              // uniform for the workgroup
    Rule u;
    int64_t L2 = 0;
    for (int j = 0; j < 3; ++j) {
        u.a[j] = c.a[j]; u.d[j] = c.b[j] - c.a[j];
        L2 += (int64_t)u.d[j] * u.d[j];
    }
    u.L2 = (uint32_t)L2;
    u.r2 = (int64_t)c.r * c.r;
    u.r2L2 = u.r2 * L2;
    const uint32_t n = S >> 1;
    // The capsule's workgroups (blockIdx.y) over its pieces: with at least one workgroup a piece, piece k has `subs` of them to
    // itself and a workgroup computes one piece box; with fewer, a workgroup takes every gridDim.y-th piece whole.  (A piece box
    // costs eight integer divisions: every workgroup walking every piece was measured at four times the whole-volume box fill
    // for one thin diagonal.)
    uint32_t subs = 1u, sub = 0u, k = blockIdx.y, k_step = gridDim.y;
    if (gridDim.y >= ps.count) {
        subs = gridDim.y / ps.count; sub = blockIdx.y % subs;
        k = blockIdx.y / subs; k_step = ps.count;
    }
    const uint64_t stride = (uint64_t)subs * blockDim.x;
    for (; k < ps.count; k += k_step) {
        uint32_t lo[3], hi[3];
        if (!vrc::stroke_piece_box(c, S, ps, k, lo, hi)) continue;
        const BoxWords b = box_words(lo, hi);
        for (uint64_t it = (uint64_t)sub * blockDim.x + threadIdx.x; it < b.items; it += stride) {
            RowWord r;
            if (!row_word(b, n, it, r)) continue;
            // z of the word's first voxel, relative to the row (negative where the word starts in the row before: n = 2)
            const int32_t z0 = 2 * (int32_t)((int64_t)(4u * r.w) - (int64_t)r.base);
            // the word's voxels span [2cx, 2cx + 1] x [2cy, 2cy + 1] x [z0, z0 + 7]: doubled centre (4cx + 1, 4cy + 1, 2 z0 + 7),
            // doubled half diagonal sqrt(1 + 1 + 49) < 8
            {
                const int64_t Q[3] = {(int64_t)(4u * r.cx + 1u) - 2 * u.a[0], (int64_t)(4u * r.cy + 1u) - 2 * u.a[1], (int64_t)(2 * z0 + 7) - 2 * u.a[2]};
                const int64_t QQ = Q[0] * Q[0] + Q[1] * Q[1] + Q[2] * Q[2], T = Q[0] * u.d[0] + Q[1] * u.d[1] + Q[2] * u.d[2];
                if (!near(u, QQ, T, 2 * (int64_t)c.r + 8)) continue;
            }
            uint32_t valid = 0u;
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint64_t byte = 4u * r.w + j;
                if (byte >= r.first && byte <= r.last) valid |= 0xffu << (8u * j);
            }
            uint32_t mask = 0u;
            for (uint32_t col = 0; col < 4u; ++col) {
                const int32_t qx = (int32_t)(2u * r.cx + (col & 1u)) - u.a[0], qy = (int32_t)(2u * r.cy + (col >> 1)) - u.a[1];
                int32_t qz = z0 - u.a[2];
                int32_t qq = qx * qx + qy * qy + qz * qz, t = qx * u.d[0] + qy * u.d[1] + qz * u.d[2];
                for (uint32_t z = 0; z < 8u; ++z) {
                    // column bit z -> word bit (z >> 1) * 8 + (z & 1) * 4 + col
                    mask |= (inside(u, qq, t) ? 1u : 0u) << ((z >> 1) * 8u + (z & 1u) * 4u + col);
                    qq += 2 * qz + 1; ++qz; t += u.d[2];
                }
            }
            mask &= valid;
            if (mask == 0xffffffffu) words[r.w] = solid ? 0xffffffffu : 0u;
            else if (mask) {
                const uint32_t have = words[r.w];
                if (solid) { if ((have & mask) != mask) atomicOr(&words[r.w], mask); }
                else if (have & mask) atomicAnd(&words[r.w], ~mask);
            }
        }
    }
}

__global__ void k_stroke_capsules(uint32_t* __restrict__ words, uint32_t S, const int32_t* __restrict__ items, uint32_t solid)
{
    const int32_t* p = items + 8ull * blockIdx.x;
    const int32_t item[8] = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]};
    if (!vrc::stroke_item_kept(item)) return;                           // uniform for the workgroup
    const vrc::Capsule c = {{item[0], item[1], item[2]}, {item[3], item[4], item[5]}, item[6]};
    fill_capsule(words, S, c, solid);
}

// centres as k_hits_to_centres leaves them: inside the volume, radius -1 for a record that is none
__global__ void k_stroke_links(uint32_t* __restrict__ words, uint32_t S, uint32_t count, const int32_t* __restrict__ centres, int32_t radius,
                               uint32_t max_gap, uint32_t solid)
{
    const int4 here = ((const int4*)centres)[blockIdx.x];
    if (here.w < 0) return;                                             // uniform for the workgroup
    vrc::Capsule c = {{here.x, here.y, here.z}, {here.x, here.y, here.z}, radius};
    if (blockIdx.x + 1u < count) {
        const int4 there = ((const int4*)centres)[blockIdx.x + 1u];
        const int64_t dx = (int64_t)there.x - here.x, dy = (int64_t)there.y - here.y, dz = (int64_t)there.z - here.z;
        const bool linked = there.w >= 0 && (max_gap == 0u || (uint64_t)(dx * dx + dy * dy + dz * dz) <= (uint64_t)max_gap * max_gap);
        if (linked) { c.b[0] = there.x; c.b[1] = there.y; c.b[2] = there.z; }
    }
    fill_capsule(words, S, c, solid);
}

}  // namespace

namespace vrc {

void stroke_capsules_run(uint32_t* words, uint32_t depth, uint64_t n, const int32_t* items, uint32_t split, uint32_t lanes, int solid, hipStream_t st)
{
    hipLaunchKernelGGL(k_stroke_capsules, dim3((uint32_t)n, split), dim3(lanes), 0, st, words, 1u << depth, items, solid ? 1u : 0u);
}

void stroke_links_run(uint32_t* words, uint32_t depth, uint64_t n, const int32_t* centres, int32_t radius, uint32_t max_gap, uint32_t split,
                      uint32_t lanes, int solid, hipStream_t st)
{
    hipLaunchKernelGGL(k_stroke_links, dim3((uint32_t)n, split), dim3(lanes), 0, st, words, 1u << depth, (uint32_t)n, centres, radius, max_gap,
                       solid ? 1u : 0u);
}

}  // namespace vrc
