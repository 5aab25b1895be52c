// vrc_sight.hip -- straight-line walks over a distance or travel field (include/vrc.h: vrc_sight_segments, vrc_sight_field).
//
// The walk.  From the centre of voxel a to the centre of voxel b, n_c = |b_c - a_c|: crossing k of axis c lies at
// t = (2k - 1) / (2 n_c), and a lane keeps e_c = 2k_c - 1 of the next crossing per axis.  t_c <= t_d is e_c n_d <= e_d n_c,
// both products below 2^21 (e <= 2047, n <= 1023), so the order and the ties are exact in 32-bit integers and no float takes
// part.  An axis that does not move (n_c = 0) compares as t = infinity by the same products, an axis that has arrived keeps
// e_c = 2 n_c + 1, a time beyond 1, so the loop needs no case for either: it runs until the n_x + n_y + n_z crossings are
// spent.  The axes of least t are the step's set T.  THIN advances all of T at once; TOUCH first visits the voxels reached
// by the proper subsets of T in ascending mask order.  Every visited voxel costs one 4-byte load at [(x*S + y)*S + z], indexed
// in 64 bits (at depth 10 the byte offset passes 2^32).  All state is in registers; no LDS, and no atomics but the two of the
// sight field's stats.
//
// The stride (DESIGN.md has the bound and its proof).  On the squared distance to a set (a field made by
// vrc_volume_distance_field; the entry points give leave for no other) with hi == 0xffffffff the value at a clear voxel p says
// that every voxel within R = isqrt(D(p)) - ceil(sqrt(lo)) of p is clear.  The walk then jumps to t' = K / n_d, the parameter
// at which the dominant axis d stands on the centre of its K-th next voxel, with every crossing at t <= t' done: axis c has
// then made floor((2 K n_c + n_d) / (2 n_d)) crossings, which is the state the plain walk has behind the event at t' (or
// behind the last one before it).  J = K - (k_d - 1) dominant crossings are taken while (2J + 1) |b - a| <= 2 (R - 2) n_d;
// |b - a| is rounded up to an integer once per walk and the quotient 2 n_d / |b - a| down to 10 fractional bits, so the jump
// only gets shorter.  A jump never takes the last dominant crossing: the walk always ends, and a blocker is always found, by a
// plain step, which is what keeps `before` exact.
#include "vrc_sight.h"

#include "vrc_group.h"

namespace {

constexpr uint32_t NONE = VRC_DISTANCE_NONE;
constexpr uint32_t GROUP = 256;               // lanes per workgroup of both kernels
constexpr uint32_t GAIN_BITS = 10;            // fractional bits of 2 n_d / |b - a|
constexpr uint32_t D_CAP = 0x3fffffu;         // a value is looked at up to here: finite ones are below 2^22, NONE is cut to it

__device__ __forceinline__ uint32_t field_at(const uint32_t* __restrict__ F, uint32_t depth, uint32_t x, uint32_t y, uint32_t z)
{
    return F[((((size_t)x << depth) | y) << depth) | z];
}

// floor(sqrt(v)) for v < 2^22
__host__ __device__ inline uint32_t isqrt22(uint32_t v)
{
    uint32_t r = 0u;
    for (int b = 10; b >= 0; --b) {
        const uint32_t t = r | (1u << b);
        if (t * t <= v) r = t;
    }
    return r;
}

// The walk a -> b, both inside the volume.  Returns whether a visited voxel was not clear; RECORD: at = that voxel (b when all
// were clear), before = the voxel visited just before `at` (`at` itself when it is a).  test_first == false leaves a itself
// untested (the sight field walks from the voxel it asks about).  gain_on: the caller's leave to stride.
template <bool RECORD>
__device__ __forceinline__ bool sight_walk(const uint32_t* __restrict__ F, uint32_t depth, uint32_t ax, uint32_t ay, uint32_t az, uint32_t bx, uint32_t by, uint32_t bz,
                                           uint32_t lo, uint32_t hi, uint32_t root_lo, bool touch, bool gain_on, bool test_first, uint32_t at[3], uint32_t before[3])
{
    const uint32_t nx = bx > ax ? bx - ax : ax - bx, ny = by > ay ? by - ay : ay - by, nz = bz > az ? bz - az : az - bz;
    const uint32_t sx = bx > ax ? 1u : 0xffffffffu, sy = by > ay ? 1u : 0xffffffffu, sz = bz > az ? 1u : 0xffffffffu;
    uint32_t x = ax, y = ay, z = az;              // the voxel the walk stands in
    uint32_t px = ax, py = ay, pz = az;           // the last visited voxel, and the one visited before it
    uint32_t qx = ax, qy = ay, qz = az;
    uint32_t ex = 1u, ey = 1u, ez = 1u, left = nx + ny + nz;
    uint32_t v = field_at(F, depth, x, y, z);
    if (test_first && (v < lo || v > hi)) {
        if (RECORD) { at[0] = before[0] = ax; at[1] = before[1] = ay; at[2] = before[2] = az; }
        return true;
    }
    // the dominant axis and 2 n_d / ceil(|b - a|) in GAIN_BITS fractional bits, rounded down; 0: this walk never strides
    const uint32_t nd = nx >= ny ? (nx >= nz ? nx : nz) : (ny >= nz ? ny : nz);
    const uint32_t dom = nx >= ny && nx >= nz ? 0u : ny >= nz ? 1u : 2u;
    uint32_t gain = 0u;
    if (gain_on && nd >= 4u) {
        const uint32_t l2 = nx * nx + ny * ny + nz * nz;      // <= 3 * 1023^2 < 2^22
        uint32_t len = isqrt22(l2);
        if (len * len < l2) ++len;
        gain = ((2u * nd) << GAIN_BITS) / len;                 // <= 2^11
    }
    while (left) {
        if (gain) {
            const uint32_t r = isqrt22(v < D_CAP ? v : D_CAP);
            if (r > root_lo + 2u) {
                const uint32_t w = ((r - root_lo - 2u) * gain) >> GAIN_BITS;     // 2J + 1 <= w; the product is below 2^22
                const uint32_t done = ((dom == 0u ? ex : dom == 1u ? ey : ez) - 1u) >> 1;      // k_d - 1
                uint32_t K = done + ((w - 1u) >> 1);
                if (K > nd - 1u) K = nd - 1u;
                if (w >= 5u && K >= done + 2u) {
                    const uint32_t den = 2u * nd;
                    const uint32_t cx = (2u * K * nx + nd) / den, cy = (2u * K * ny + nd) / den, cz = (2u * K * nz + nd) / den;
                    x = ax + sx * cx; y = ay + sy * cy; z = az + sz * cz;
                    ex = 2u * cx + 1u; ey = 2u * cy + 1u; ez = 2u * cz + 1u;
                    left = (nx - cx) + (ny - cy) + (nz - cz);       // the dominant axis keeps a crossing: never 0
                    px = x; py = y; pz = z;
                    v = field_at(F, depth, x, y, z);                // clear by the bound; read for the next radius
                    continue;
                }
            }
        }
        const uint32_t xy = ex * ny, yx = ey * nx, xz = ex * nz, zx = ez * nx, yz = ey * nz, zy = ez * ny;
        const uint32_t T = (xy <= yx && xz <= zx ? 1u : 0u) | (yx <= xy && yz <= zy ? 2u : 0u) | (zx <= xz && zy <= yz ? 4u : 0u);
        if (touch && (T & (T - 1u))) {
            for (uint32_t sub = 1u; sub < 7u; ++sub) {
                if ((sub & ~T) || sub == T) continue;
                const uint32_t tx = x + (sub & 1u ? sx : 0u), ty = y + (sub & 2u ? sy : 0u), tz = z + (sub & 4u ? sz : 0u);
                v = field_at(F, depth, tx, ty, tz);
                qx = px; qy = py; qz = pz;
                px = tx; py = ty; pz = tz;
                if (v < lo || v > hi) {
                    if (RECORD) { at[0] = px; at[1] = py; at[2] = pz; before[0] = qx; before[1] = qy; before[2] = qz; }
                    return true;
                }
            }
        }
        x += T & 1u ? sx : 0u; y += T & 2u ? sy : 0u; z += T & 4u ? sz : 0u;
        ex += T & 1u ? 2u : 0u; ey += T & 2u ? 2u : 0u; ez += T & 4u ? 2u : 0u;
        left -= __popc(T);
        v = field_at(F, depth, x, y, z);
        qx = px; qy = py; qz = pz;
        px = x; py = y; pz = z;
        if (v < lo || v > hi) {
            if (RECORD) { at[0] = px; at[1] = py; at[2] = pz; before[0] = qx; before[1] = qy; before[2] = qz; }
            return true;
        }
    }
    if (RECORD) { at[0] = px; at[1] = py; at[2] = pz; before[0] = qx; before[1] = qy; before[2] = qz; }
    return false;
}

// a lane per segment
__global__ __launch_bounds__(GROUP) void k_sight_segments(const uint32_t* __restrict__ F, uint32_t depth, uint64_t count, const int32_t* __restrict__ segments,
                                                          uint32_t lo, uint32_t hi, uint32_t root_lo, uint32_t touch, uint32_t stride, vrc_sight* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * GROUP + threadIdx.x;
    if (i >= count) return;
    const uint32_t S = 1u << depth;
    const int32_t* s = segments + 6u * i;
    const uint32_t ax = (uint32_t)s[0], ay = (uint32_t)s[1], az = (uint32_t)s[2], bx = (uint32_t)s[3], by = (uint32_t)s[4], bz = (uint32_t)s[5];
    vrc_sight rec = {};
    if (ax < S && ay < S && az < S && bx < S && by < S && bz < S) {      // a negative coordinate is a large unsigned one
        const bool blocked = sight_walk<true>(F, depth, ax, ay, az, bx, by, bz, lo, hi, root_lo, touch != 0u, stride != 0u, true, rec.at, rec.before);
        rec.status = blocked ? VRC_SIGHT_BLOCKED : VRC_SIGHT_CLEAR;
    } else {
        rec.status = VRC_SIGHT_OUTSIDE;
    }
    out[i] = rec;
}

// A lane per voxel p, consecutive lanes consecutive z; the walk runs p -> eye, so the lanes of a wave converge on the same
// voxels, and p itself is not tested.  Every wave reduces its count and its packed maximum by shuffles and issues at most two
// 64-bit vector atomics.
__global__ __launch_bounds__(GROUP) void k_sight_field(const uint32_t* __restrict__ F, uint32_t depth, uint32_t eye_x, uint32_t eye_y, uint32_t eye_z, uint32_t r2,
                                                       uint32_t lo, uint32_t hi, uint32_t root_lo, uint32_t touch, uint32_t stride, uint32_t* __restrict__ out,
                                                       unsigned long long* __restrict__ stats)
{
    const size_t i = (size_t)blockIdx.x * GROUP + threadIdx.x, total = (size_t)1u << (3u * depth);
    const uint32_t mask = (1u << depth) - 1u;
    uint32_t value = NONE;
    if (i < total) {
        const uint32_t x = (uint32_t)(i >> (2u * depth)), y = (uint32_t)(i >> depth) & mask, z = (uint32_t)i & mask;
        const uint32_t dx = x > eye_x ? x - eye_x : eye_x - x, dy = y > eye_y ? y - eye_y : eye_y - y, dz = z > eye_z ? z - eye_z : eye_z - z;
        const uint32_t d2 = dx * dx + dy * dy + dz * dz;
        if (d2 == 0u) {
            value = 0u;
        } else if (d2 <= r2) {
            uint32_t at[3], before[3];
            if (!sight_walk<false>(F, depth, x, y, z, eye_x, eye_y, eye_z, lo, hi, root_lo, touch != 0u, stride != 0u, false, at, before)) value = d2;
        }
        out[i] = value;
    }
    const uint32_t seen = wave_sum(value != NONE ? 1u : 0u);
    unsigned long long best = value != NONE ? ((unsigned long long)value << 32) | (uint32_t)~(uint32_t)i : 0ull;
    for (int o = 32; o; o >>= 1) {
        const unsigned long long t = __shfl_xor(best, o);
        best = t > best ? t : best;
    }
    if ((threadIdx.x & 63u) == 0u && seen) {
        atomicAdd(&stats[0], (unsigned long long)seen);
        atomicMax(&stats[1], best);
    }
}

}  // namespace

namespace vrc {

uint32_t sight_root_above(uint32_t lo)
{
    uint32_t c = 0u;
    for (int b = 15; b >= 0; --b) {
        const uint32_t t = c | (1u << b);
        if ((uint64_t)t * t <= lo) c = t;
    }
    return (uint64_t)c * c < lo ? c + 1u : c;
}

void sight_segments_run(const uint32_t* field, uint32_t depth, uint64_t n, const int32_t* segments, uint32_t lo, uint32_t hi, bool touch, bool stride,
                        vrc_sight* out, hipStream_t st)
{
    hipLaunchKernelGGL(k_sight_segments, dim3((uint32_t)((n + GROUP - 1u) / GROUP)), dim3(GROUP), 0, st, field, depth, n, segments, lo, hi, sight_root_above(lo),
                       touch ? 1u : 0u, stride ? 1u : 0u, out);
}

void sight_field_run(const uint32_t* field, uint32_t depth, const uint32_t eye[3], uint32_t radius, uint32_t lo, uint32_t hi, bool touch, bool stride,
                     uint32_t* out, unsigned long long* stats, hipStream_t st)
{
    // squared distances in the volume are below 2^22: a radius of 2048 and more, like none, takes every voxel
    const uint32_t r2 = radius == 0u || radius >= 2048u ? NONE : radius * radius;
    const size_t total = (size_t)1u << (3u * depth);
    hipLaunchKernelGGL(k_sight_field, dim3((uint32_t)((total + GROUP - 1u) / GROUP)), dim3(GROUP), 0, st, field, depth, eye[0], eye[1], eye[2], r2, lo, hi,
                       sight_root_above(lo), touch ? 1u : 0u, stride ? 1u : 0u, out, stats);
}

}  // namespace vrc
