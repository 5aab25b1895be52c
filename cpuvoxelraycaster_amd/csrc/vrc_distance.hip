// vrc_distance.hip -- the exact squared Euclidean distance field of the editable volume's bit field (include/vrc.h:
// vrc_volume_distance_field, vrc_distance_*).
//
// D(p) = min over the feature voxels q of |p - q|^2 is separable: with g0(x, y, z) = the squared distance to the nearest
// feature voxel of the same z column, g1(x, y, z) = min_j g0(x, j, z) + (y - j)^2 and D(x, y, z) = min_j g1(j, y, z) +
// (x - j)^2.  Everything is an integer below 2^23; "no feature in this line" is the sentinel VRC_DISTANCE_NONE, which is
// tested for and never added to.  The field is dense, [(x*S + y)*S + z], and the three passes work in place on it, one
// kernel each on one stream; no workgroup waits for another.
//
//   z   k_distance_z: a workgroup takes 256 / S columns (2048 / S from 256^3 on) at a time.  The column's bits (S / 32 words) are
//       assembled from the brick bytes into LDS, one lane per word, the words' nearest feature below and above follow from
//       one serial walk over at most 32 words, and then a lane per voxel finds its nearest feature with one count of
//       leading and one of trailing zeros on its own word, falling back on the word tables.  The features are counted on
//       the way (popcount per word, LDS reduction, one 64-bit atomic per workgroup).
//   y,x k_distance_minplus<1 / 0>: out[i] = min_j in[j] + (i - j)^2 along a line by the LOWER-ENVELOPE STACK (Felzenszwalb
//       and Huttenlocher; Meijster's scan is the same idea): one walk over the line keeps the parabolas that are lowest
//       somewhere, a second walk reads the minimum off them with a pointer that only moves forward.  2 S steps per line
//       whatever the input -- the monotone-argmin divide and conquer would be S log S with a recursion per lane, and a
//       search around each voxel is unbounded (2^40 steps for one voxel in 1024^3).  A parabola is popped when its
//       crossover with the one below is not left of its crossover with the newcomer; the two quotients are compared by
//       cross-multiplication in 64 bits, so no division and no float takes part, and the boundaries need not be stored: the
//       second walk compares neighbouring parabolas at i directly, which is exact.  A stack entry is (f << 10) | j in 32
//       bits (f < 2^22, j < 2^10).  A lane owns a line and the lanes of a wave are consecutive z, so every step of both
//       walks reads or writes one contiguous row of the field; a lane reads its whole line before it writes any of it, so
//       the pass is in place.  The stacks are [entry][lane]: in LDS up to 128^3 (64 lanes x S entries x 4 bytes <= 32 KiB),
//       from 256^3 on in a device block sized by the lines in flight (8 waves per compute unit, looping over the lines).
//       The x pass also applies the wall term of `outside` and reduces the stats: (d2 << 32) | ~dense index is monotone
//       in "larger distance, then smaller index", so a maximum per workgroup in LDS and one 64-bit vector atomicMax per
//       workgroup give a result that does not depend on scheduling.
#include "vrc_distance.h"

#include "vrc_box_words.h"
#include "vrc_word_columns.h"

namespace {

constexpr uint32_t NONE = VRC_DISTANCE_NONE;
constexpr uint32_t GROUP = 256;               // lanes per workgroup of the z pass, at and select
constexpr uint32_t LANES = 64;                // lines per workgroup of the min-plus passes: one wave
constexpr uint32_t LDS_STACK_MAX_DEPTH = 7;   // 64 x 128 x 4 bytes = 32 KiB
constexpr uint32_t WAVES_PER_CU = 8;          // lines in flight = compute units x 8 x 64

// columns a workgroup of the z pass takes per step: a lane per voxel up to 128^3, above that as many columns as the 64
// words of bits in LDS hold (8, 4, 2 at 256^3, 512^3, 1024^3), a lane looping over their voxels
__host__ __device__ inline uint32_t z_columns_per_step(uint32_t S) { return S >= GROUP ? 2048u / S : GROUP / S; }

__global__ __launch_bounds__(GROUP) void k_distance_z(const uint32_t* __restrict__ words, uint32_t depth, uint32_t flip, uint32_t* __restrict__ D,
                                                      unsigned long long* __restrict__ stats)
{
    __shared__ uint32_t bits[64], below[64], above[64], part[GROUP];
    const uint32_t S = 1u << depth, n = S >> 1, columns = S * S, t = threadIdx.x;
    const uint32_t wpc = S >= 32u ? S >> 5 : 1u;               // words of bits per column
    const uint32_t cpi = z_columns_per_step(S);                // columns per step; cpi * wpc <= 64
    uint32_t features = 0u;
    for (uint32_t col0 = blockIdx.x * cpi; col0 < columns; col0 += gridDim.x * cpi) {      // uniform for the workgroup
        if (t < cpi * wpc) {
            const uint32_t c = col0 + t / wpc, k = t % wpc;
            uint32_t w = 0u;
            if (c < columns) {
                const uint32_t x = c >> depth, y = c & (S - 1u), sh = (y & 1u) * 2u + (x & 1u);
                const uint32_t row = ((x >> 1) * n + (y >> 1)) * n;                          // byte index of brick (cx, cy, 0)
                if (n >= 16u) {                                                             // 16 bricks = 4 aligned words
                    const uint4 q = *(const uint4*)(words + ((row + 16u * k) >> 2));
                    w = column_bits_of_word(q.x, sh) | (column_bits_of_word(q.y, sh) << 8) | (column_bits_of_word(q.z, sh) << 16) |
                        (column_bits_of_word(q.w, sh) << 24);
                    w ^= flip;
                } else {
                    const uint8_t* b = (const uint8_t*)words + row;
                    for (uint32_t j = 0; j < n; ++j) {
                        const uint32_t v = b[j] >> sh;
                        w |= ((v & 1u) | ((v >> 3) & 2u)) << (2u * j);
                    }
                    w = (w ^ flip) & ((1u << S) - 1u);
                }
                features += __popc(w);
            }
            bits[t] = w;
        }
        __syncthreads();
        if (t < cpi) {                                           // the nearest feature in the words below / above each word
            uint32_t last = NONE;
            for (uint32_t k = 0; k < wpc; ++k) {
                const uint32_t w = bits[t * wpc + k];
                below[t * wpc + k] = last;
                if (w) last = 32u * k + 31u - (uint32_t)__clz(w);
            }
            last = NONE;
            for (uint32_t k = wpc; k-- > 0u;) {
                const uint32_t w = bits[t * wpc + k];
                above[t * wpc + k] = last;
                if (w) last = 32u * k + (uint32_t)__ffs(w) - 1u;
            }
        }
        __syncthreads();
        for (uint32_t v = t; v < cpi * S; v += GROUP) {
            const uint32_t lc = v >> depth, z = v & (S - 1u), c = col0 + lc;
            if (c >= columns) break;
            const uint32_t slot = lc * wpc + (z >> 5), b = z & 31u, w = bits[slot];
            const uint32_t lo = w & (0xffffffffu >> (31u - b)), hi = w & (0xffffffffu << b);
            const uint32_t zb = lo ? (z & ~31u) + 31u - (uint32_t)__clz(lo) : below[slot];
            const uint32_t za = hi ? (z & ~31u) + (uint32_t)__ffs(hi) - 1u : above[slot];
            uint32_t d = NONE;
            if (zb != NONE) d = z - zb;
            if (za != NONE && za - z < d) d = za - z;
            D[c * S + z] = d == NONE ? NONE : d * d;
        }
        __syncthreads();
    }
    // Kept as the LDS tree it was: with group_sum (vrc_group.h) the to = SOLID field rows of tools/bench_edit.py --distance
    // came out 0.5 - 2.4 % slower than the parent, beyond the parent's run-to-run spread (docs/NOTEBOOK.md).
    part[t] = features;                                          // at most 2^20 x 2^10 / gridDim per workgroup: fits
    __syncthreads();
    for (uint32_t s = GROUP / 2u; s; s >>= 1) {
        if (t < s) part[t] += part[t + s];
        __syncthreads();
    }
    if (t == 0 && part[0]) atomicAdd(&stats[0], (unsigned long long)part[0]);
}

// AXIS 1: the lines along y, line l = x * S + z.  AXIS 0: the lines along x, l = y * S + z, the last pass.
template <int AXIS, bool IN_LDS>
__global__ __launch_bounds__(LANES) void k_distance_minplus(uint32_t* D, uint32_t depth, uint32_t* stacks, uint32_t outside, unsigned long long* stats)
{
    extern __shared__ uint32_t lds_stacks[];
    __shared__ unsigned long long red[LANES];
    const uint32_t S = 1u << depth, lines = S * S, lane = threadIdx.x;
    const uint32_t sh = AXIS == 1 ? depth : 2u * depth;          // log2 of the step along the line
    uint32_t* stk;                                               // entry k of this lane: stk[k * LANES]
    if (IN_LDS) stk = lds_stacks + lane;
    else stk = stacks + (size_t)blockIdx.x * LANES * S + lane;
    unsigned long long best = 0ull;
    for (uint32_t l0 = blockIdx.x * LANES; l0 < lines; l0 += gridDim.x * LANES) {
        const uint32_t l = l0 + lane;
        if (l >= lines) break;                                   // 4^3 only: 16 lines
        const uint32_t base = AXIS == 1 ? (((l >> depth) << (2u * depth)) | (l & (S - 1u))) : l;
        uint32_t* line = D + base;
        // first walk: the parabolas of the lower envelope, left to right; (va, Fa) and (vb, Fb) mirror the two topmost
        // entries, F = f + v^2
        uint32_t top = 0u;
        int32_t va = 0, Fa = 0, vb = 0, Fb = 0;
        for (uint32_t j0 = 0; j0 < S; j0 += 4u) {
            uint32_t f4[4];
            for (uint32_t u = 0; u < 4u; ++u) f4[u] = line[(size_t)(j0 + u) << sh];
            for (uint32_t u = 0; u < 4u; ++u) {
                const uint32_t f = f4[u];
                if (f == NONE) continue;
                const int32_t q = (int32_t)(j0 + u), Fq = (int32_t)f + q * q;
                // b is lowest nowhere once crossover(a, b) >= crossover(b, q):
                // (Fb - Fa) / (vb - va) >= (Fq - Fb) / (q - vb), both denominators positive
                while (top >= 2u && (int64_t)(Fb - Fa) * (q - vb) >= (int64_t)(Fq - Fb) * (vb - va)) {
                    --top;
                    vb = va; Fb = Fa;
                    if (top >= 2u) {
                        const uint32_t e = stk[(top - 2u) * LANES];
                        va = (int32_t)(e & 1023u); Fa = (int32_t)(e >> 10) + va * va;
                    }
                }
                stk[top * LANES] = (f << 10) | (uint32_t)q;
                va = vb; Fa = Fb; vb = q; Fb = Fq;
                ++top;
            }
        }
        // second walk: the envelope's value at i; the pointer only moves forward
        uint32_t k = 0u;
        int32_t vc = 0, fc = 0, vn = 0, fn = 0;
        if (top) { const uint32_t e = stk[0]; vc = (int32_t)(e & 1023u); fc = (int32_t)(e >> 10); }
        if (top > 1u) { const uint32_t e = stk[LANES]; vn = (int32_t)(e & 1023u); fn = (int32_t)(e >> 10); }
        const uint32_t py = l >> depth, pz = l & (S - 1u);       // AXIS 0: the voxel is (i, py, pz)
        uint32_t wall_yz = 0u;
        if (AXIS == 0 && outside) {
            const uint32_t wy = py + 1u < S - py ? py + 1u : S - py, wz = pz + 1u < S - pz ? pz + 1u : S - pz;
            wall_yz = wy < wz ? wy : wz;
        }
        for (uint32_t i = 0; i < S; ++i) {
            uint32_t out = NONE;
            if (top) {
                int32_t d = (int32_t)i - vc;
                uint32_t val = (uint32_t)(fc + d * d);
                while (k + 1u < top) {
                    d = (int32_t)i - vn;
                    const uint32_t next = (uint32_t)(fn + d * d);
                    if (next > val) break;
                    ++k; vc = vn; fc = fn; val = next;
                    if (k + 1u < top) { const uint32_t e = stk[(k + 1u) * LANES]; vn = (int32_t)(e & 1023u); fn = (int32_t)(e >> 10); }
                }
                out = val;
            }
            if (AXIS == 0) {
                if (outside) {
                    uint32_t w = i + 1u < S - i ? i + 1u : S - i;
                    w = w < wall_yz ? w : wall_yz;
                    if (w * w < out) out = w * w;
                }
                if (out != NONE) {
                    const unsigned long long packed = ((unsigned long long)out << 32) | (uint32_t)~(base + (i << sh));
                    best = packed > best ? packed : best;
                }
            }
            line[(size_t)i << sh] = out;
        }
    }
    if (AXIS == 0) {
        red[lane] = best;
        __syncthreads();
        for (uint32_t s = LANES / 2u; s; s >>= 1) {
            if (lane < s && red[lane + s] > red[lane]) red[lane] = red[lane + s];
            __syncthreads();
        }
        if (lane == 0 && red[0]) atomicMax(&stats[1], red[0]);
    }
}

__global__ void k_distance_at(const uint32_t* __restrict__ D, uint32_t depth, uint64_t count, const uint32_t* __restrict__ xyz, uint32_t* __restrict__ d2)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t S = 1u << depth, x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    d2[i] = x < S && y < S && z < S ? D[(((size_t)x << depth | y) << depth) | z] : NONE;
}

// One thread per occupancy word = 4 bricks along z = 2 x 2 x 8 voxels: four runs of eight consecutive field entries.  The
// word is written whole with a plain store: it has one owner.  4^3 (two brick rows to a word) reads voxel by voxel.
__global__ __launch_bounds__(GROUP) void k_distance_select(const uint32_t* __restrict__ D, uint32_t depth, uint32_t lo, uint32_t hi, uint32_t* __restrict__ dst, int op)
{
    const uint32_t S = 1u << depth, lg = depth - 1u, n = S >> 1, n_words = 1u << (3u * lg - 2u);
    const uint32_t w = blockIdx.x * GROUP + threadIdx.x;
    if (w >= n_words) return;
    uint32_t K = 0u;
    if (n >= 4u) {
        const uint32_t B = 4u * w, cz = B & (n - 1u), cy = (B >> lg) & (n - 1u), cx = B >> (2u * lg);
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t x = 2u * cx + (k & 1u), y = 2u * cy + (k >> 1);
            const uint4* run = (const uint4*)(D + ((((size_t)x << depth | y) << depth) | (2u * cz)));
            const uint4 a = run[0], b = run[1];
            const uint32_t v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            for (uint32_t zz = 0; zz < 8u; ++zz)
                K |= (lo <= v[zz] && v[zz] <= hi ? 1u : 0u) << (8u * (zz >> 1) + (zz & 1u) * 4u + k);
        }
    } else {
        for (uint32_t bit = 0; bit < 32u; ++bit) {
            const uint32_t B = 4u * w + (bit >> 3), cz = B & 1u, cy = (B >> 1) & 1u, cx = B >> 2;
            const uint32_t x = 2u * cx + (bit & 1u), y = 2u * cy + ((bit >> 1) & 1u), z = 2u * cz + ((bit >> 2) & 1u);
            const uint32_t v = D[(x * S + y) * S + z];
            K |= (lo <= v && v <= hi ? 1u : 0u) << bit;
        }
    }
    store_selected_word(dst, w, K, op);
}

uint32_t minplus_groups(uint32_t depth, int cu_count)
{
    const uint32_t lines = 1u << (2u * depth);
    const uint32_t want = (lines + LANES - 1u) / LANES, cap = (uint32_t)(cu_count > 0 ? cu_count : 1) * WAVES_PER_CU;
    return want < cap ? want : cap;
}

}  // namespace

namespace vrc {

size_t distance_scratch_bytes(uint32_t depth, int cu_count)
{
    const size_t stacks = depth > LDS_STACK_MAX_DEPTH ? ((size_t)minplus_groups(depth, cu_count) * LANES * 4u) << depth : 0u;
    return 16u + stacks;
}

unsigned long long* distance_stats_slots(uint32_t* scratch) { return (unsigned long long*)scratch; }

void distance_run(const uint32_t* medium, uint32_t depth, int to, int outside, int cu_count, uint32_t* field, uint32_t* scratch, hipStream_t st)
{
    unsigned long long* stats = distance_stats_slots(scratch);
    uint32_t* stacks = scratch + 4;
    (void)hipMemsetAsync(stats, 0, 16, st);
    const uint32_t S = 1u << depth, cpi = z_columns_per_step(S);
    uint32_t z_groups = (S * S + cpi - 1u) / cpi;
    const uint32_t z_cap = (uint32_t)(cu_count > 0 ? cu_count : 1) * 16u;
    if (z_groups > z_cap) z_groups = z_cap;
    hipLaunchKernelGGL(k_distance_z, dim3(z_groups), dim3(GROUP), 0, st, medium, depth, to ? 0xffffffffu : 0u, field, stats);
    const dim3 grid(minplus_groups(depth, cu_count)), block(LANES);
    if (depth <= LDS_STACK_MAX_DEPTH) {
        const size_t lds = ((size_t)LANES * 4u) << depth;
        hipLaunchKernelGGL((k_distance_minplus<1, true>), grid, block, lds, st, field, depth, nullptr, 0u, stats);
        hipLaunchKernelGGL((k_distance_minplus<0, true>), grid, block, lds, st, field, depth, nullptr, outside ? 1u : 0u, stats);
    } else {
        hipLaunchKernelGGL((k_distance_minplus<1, false>), grid, block, 0, st, field, depth, stacks, 0u, stats);
        hipLaunchKernelGGL((k_distance_minplus<0, false>), grid, block, 0, st, field, depth, stacks, outside ? 1u : 0u, stats);
    }
}

void distance_at_run(const uint32_t* field, uint32_t depth, uint64_t n, const uint32_t* xyz, uint32_t* d2, hipStream_t st)
{
    hipLaunchKernelGGL(k_distance_at, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, field, depth, n, xyz, d2);
}

void distance_select_run(const uint32_t* field, uint32_t depth, uint32_t lo, uint32_t hi, uint32_t* dst, int op, hipStream_t st)
{
    const uint32_t n_words = 1u << (3u * (depth - 1u) - 2u);
    hipLaunchKernelGGL(k_distance_select, dim3((n_words + GROUP - 1u) / GROUP), dim3(GROUP), 0, st, field, depth, lo, hi, dst, op);
}

}  // namespace vrc
