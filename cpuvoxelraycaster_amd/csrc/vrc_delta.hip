// vrc_delta.hip -- the difference of two occupancy fields as a list of changed words, and its application (include/vrc.h:
// vrc_delta_diff, vrc_delta_create, vrc_delta_apply): the undo / redo step and what a replica needs of an edit.
//
// A record is {word, bits}: bits = before[word] ^ after[word] != 0, in strictly ascending word.  The layout of a word
// (2 x 2 x 8 voxels, bit zz*4 + yb*2 + xb) is described at the top of vrc_flood.hip; the masks are vrc_flood.h's.
//
// The diff is three passes on one stream over a = before and b = after.  A workgroup is ONE wave of 64 lanes and takes 256
// consecutive words, a lane four consecutive words with one 16-byte load from each field; no workgroup waits for another:
//   1. count: the changed words of the workgroup into its slot; the changed voxels and their box, reduced across the wave
//             with shuffles (a one-wave workgroup has nothing to pass through LDS), leave it as one 64-bit atomicAdd and
//             at most six 32-bit atomicMin / atomicMax -- an atomic on a bound is left out where the bound read beforehand
//             is already as wide, which is safe because a bound only ever widens;
//   2. scan:  one workgroup walks the slots 1024 at a time and replaces them by their exclusive prefix (scan_slots);
//   3. emit:  a workgroup with an empty range leaves after reading two slots.  The others read their words again, prefix
//             the per-lane counts across the wave, and every lane writes its records, one 8-byte store each.
// Each of passes 1 and 3 reads both fields once and nothing else.  Word and record indices reach 2^25 and stay 32-bit; the
// voxel count is 64-bit.
//
// The box of a word follows from its index and mask tests on its bits, no voxel is expanded: WORD_X0 / WORD_X1 and
// WORD_Y0 / WORD_Y1 say which of the brick's two x and y are present, the lowest and highest set nibble give z.  At 4^3 a
// word holds two brick ROWS (bricks (cx, 0, 0) (cx, 0, 1) (cx, 1, 0) (cx, 1, 1)), so the nibble index is 4 cy + z there:
// that size has a branch of its own (word_box), as vrc_surface.hip's word_masks has.
#include "vrc_delta.h"

#include "vrc_flood.h"
#include "vrc_group.h"

namespace {

using vrc::DeltaTotals;
using vrc::WORD_X0;
using vrc::WORD_X1;
using vrc::WORD_Y0;
using vrc::WORD_Y1;

constexpr uint32_t LANES = 64;                // one wave per workgroup
constexpr uint32_t GROUP = 4u * LANES;        // words per workgroup

// the voxels of a lane's records: how many, and their box with hi INCLUSIVE (lo > hi: none yet)
struct Extent {
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
    uint32_t hi[3] = {0u, 0u, 0u};
    unsigned long long voxels = 0ull;
};

// widens e by the voxels `bits` (!= 0) of word W; lg = log2 of the bricks per axis
__device__ __forceinline__ void word_box(uint32_t W, uint32_t bits, uint32_t lg, Extent& e)
{
    uint32_t l[3], h[3];
    if (lg >= 2u) {
        // n >= 4: word (cx, cy, wz) of n / 4 words along z, nibble k = z - 8 wz
        const uint32_t lgz = lg - 2u, nm = (1u << lg) - 1u;
        const uint32_t wz = W & ((1u << lgz) - 1u), cy = (W >> lgz) & nm, cx = W >> (lgz + lg);
        l[0] = 2u * cx + ((bits & WORD_X0) ? 0u : 1u);
        h[0] = 2u * cx + ((bits & WORD_X1) ? 1u : 0u);
        l[1] = 2u * cy + ((bits & WORD_Y0) ? 0u : 1u);
        h[1] = 2u * cy + ((bits & WORD_Y1) ? 1u : 0u);
        l[2] = 8u * wz + ((uint32_t)(__ffs((int)bits) - 1) >> 2);
        h[2] = 8u * wz + ((31u - (uint32_t)__clz((int)bits)) >> 2);
    } else {
        // 4^3: word cx, its low half the brick row cy = 0 and its high half cy = 1; nibble k of a half = z
        const uint32_t h0 = bits & 0xffffu, h1 = bits >> 16, z = h0 | h1;
        l[0] = 2u * W + ((bits & WORD_X0) ? 0u : 1u);
        h[0] = 2u * W + ((bits & WORD_X1) ? 1u : 0u);
        l[1] = h0 ? ((h0 & WORD_Y0) ? 0u : 1u) : ((h1 & WORD_Y0) ? 2u : 3u);
        h[1] = h1 ? ((h1 & WORD_Y1) ? 3u : 2u) : ((h0 & WORD_Y1) ? 1u : 0u);
        l[2] = (uint32_t)(__ffs((int)z) - 1) >> 2;
        h[2] = (31u - (uint32_t)__clz((int)z)) >> 2;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e.lo[a] = min(e.lo[a], l[a]);
        e.hi[a] = max(e.hi[a], h[a]);
    }
    e.voxels += (uint32_t)__popc(bits);
}

// e reduced over the wave; lane 0 adds it to the totals (hi becomes exclusive there)
__device__ __forceinline__ void publish(Extent e, DeltaTotals* __restrict__ totals)
{
    for (int o = 32; o; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            e.lo[a] = min(e.lo[a], (uint32_t)__shfl_down(e.lo[a], o));
            e.hi[a] = max(e.hi[a], (uint32_t)__shfl_down(e.hi[a], o));
        }
        e.voxels += (unsigned long long)__shfl_down(e.voxels, o);
    }
    if ((threadIdx.x & 63u) != 0u || !e.voxels) return;
    atomicAdd(&totals->voxels, e.voxels);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // a stale read can only show a narrower bound than the current one: then the atomic runs and changes nothing
        if (e.lo[a] < __hip_atomic_load(&totals->lo[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&totals->lo[a], e.lo[a]);
        if (e.hi[a] + 1u > __hip_atomic_load(&totals->hi[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&totals->hi[a], e.hi[a] + 1u);
    }
}

// a[W0 .. W0 + 4) ^ b[W0 .. W0 + 4), 0 from n_words on.  n_words is a power of two: only the two words of 4^3 end inside a
// lane's four, everywhere else a lane is wholly inside (one 16-byte load per field) or wholly outside.
__device__ __forceinline__ uint4 changed_words(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t W0, uint32_t n_words)
{
    uint4 x = make_uint4(0u, 0u, 0u, 0u);
    if (W0 + 4u <= n_words) {
        const uint4 p = *(const uint4*)(a + W0), q = *(const uint4*)(b + W0);
        x = make_uint4(p.x ^ q.x, p.y ^ q.y, p.z ^ q.z, p.w ^ q.w);
    } else if (W0 < n_words) {
        x.x = a[W0] ^ b[W0];
        if (W0 + 1u < n_words) x.y = a[W0 + 1u] ^ b[W0 + 1u];
        if (W0 + 2u < n_words) x.z = a[W0 + 2u] ^ b[W0 + 2u];
    }
    return x;
}

__global__ __launch_bounds__(LANES) void k_delta_count(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t n_words, uint32_t lg,
                                                       uint32_t* __restrict__ slots, DeltaTotals* __restrict__ totals)
{
    __shared__ uint32_t part[1];
    const uint32_t W0 = blockIdx.x * GROUP + 4u * threadIdx.x;
    const uint4 x = changed_words(a, b, W0, n_words);
    const uint32_t mine = (x.x ? 1u : 0u) + (x.y ? 1u : 0u) + (x.z ? 1u : 0u) + (x.w ? 1u : 0u);
    const uint32_t all = group_sum<1u>(mine, part);
    if (threadIdx.x == 0) slots[blockIdx.x] = all;
    if (!all) return;                                                   // uniform for the workgroup
    Extent e;
    if (x.x) word_box(W0, x.x, lg, e);
    if (x.y) word_box(W0 + 1u, x.y, lg, e);
    if (x.z) word_box(W0 + 2u, x.z, lg, e);
    if (x.w) word_box(W0 + 3u, x.w, lg, e);
    publish(e, totals);
}

__global__ __launch_bounds__(LANES) void k_delta_emit(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t n_words,
                                                      const uint32_t* __restrict__ slots, uint2* __restrict__ records)
{
    __shared__ uint32_t part[1];
    const uint32_t from = slots[blockIdx.x], to = slots[blockIdx.x + 1u];
    if (from == to) return;                                             // uniform for the workgroup
    const uint32_t W0 = blockIdx.x * GROUP + 4u * threadIdx.x;
    const uint4 x = changed_words(a, b, W0, n_words);
    const uint32_t mine = (x.x ? 1u : 0u) + (x.y ? 1u : 0u) + (x.z ? 1u : 0u) + (x.w ? 1u : 0u);
    uint32_t all = 0u;
    uint32_t at = from + group_exclusive_scan<1u>(mine, part, &all);    // at + mine <= to <= the records allocated ...
    // ... as long as nobody edits a field between the passes; held to `to` all the same, so that such a misuse cannot write
    // beyond the allocation
    if (x.x && at < to) records[at++] = make_uint2(W0, x.x);
    if (x.y && at < to) records[at++] = make_uint2(W0 + 1u, x.y);
    if (x.z && at < to) records[at++] = make_uint2(W0 + 2u, x.z);
    if (x.w && at < to) records[at] = make_uint2(W0 + 3u, x.w);
}

// one lane per caller record: the rule of a list, and the extent of the records that keep it
__global__ __launch_bounds__(LANES) void k_delta_check(const uint2* __restrict__ records, uint32_t n, uint32_t n_words, uint32_t lg,
                                                       DeltaTotals* __restrict__ totals)
{
    const uint32_t i = blockIdx.x * LANES + threadIdx.x;
    Extent e;
    if (i < n) {
        const uint2 r = records[i];
        const bool bad = r.y == 0u || r.x >= n_words || (i && records[i - 1u].x >= r.x);
        if (bad)
            atomicMin(&totals->first_bad, i);
        else
            word_box(r.x, r.y, lg, e);
    }
    publish(e, totals);
}

__global__ __launch_bounds__(256) void k_delta_apply(const uint2* __restrict__ records, uint32_t n, uint32_t* __restrict__ words)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint2 r = records[i];
    words[r.x] ^= r.y;                                                  // the words of a list are distinct: this lane's alone
}

uint32_t groups_of(uint32_t depth) { return (vrc::delta_words(depth) + GROUP - 1u) / GROUP; }
uint32_t* slots_of(void* scratch) { return (uint32_t*)((DeltaTotals*)scratch + 1); }

}  // namespace

namespace vrc {

size_t delta_scratch_bytes(uint32_t depth) { return sizeof(DeltaTotals) + ((size_t)groups_of(depth) + 1u) * 4u; }

void delta_totals_reset(DeltaTotals* totals, hipStream_t st)
{
    (void)hipMemsetAsync(totals, 0xff, 16, st);                         // lo and first_bad
    (void)hipMemsetAsync((uint8_t*)totals + 16, 0, sizeof(DeltaTotals) - 16u, st);
}

void delta_offsets_run(const uint32_t* before, const uint32_t* after, uint32_t depth, void* scratch, hipStream_t st)
{
    DeltaTotals* totals = (DeltaTotals*)scratch;
    delta_totals_reset(totals, st);
    hipLaunchKernelGGL(k_delta_count, dim3(groups_of(depth)), dim3(LANES), 0, st, before, after, delta_words(depth), depth - 1u, slots_of(scratch), totals);
    // a slot <= 256, the total <= 2^25; the total also goes into totals->words
    hipLaunchKernelGGL(k_scan_slots<uint32_t>, dim3(1), dim3(SCAN_GROUP), 0, st, slots_of(scratch), groups_of(depth), &totals->words);
}

void delta_emit_run(const uint32_t* before, const uint32_t* after, uint32_t depth, const void* scratch, uint2* records, hipStream_t st)
{
    hipLaunchKernelGGL(k_delta_emit, dim3(groups_of(depth)), dim3(LANES), 0, st, before, after, delta_words(depth), slots_of((void*)scratch), records);
}

void delta_check_run(const uint2* records, uint32_t n, uint32_t depth, DeltaTotals* totals, hipStream_t st)
{
    delta_totals_reset(totals, st);
    if (n) hipLaunchKernelGGL(k_delta_check, dim3((n + LANES - 1u) / LANES), dim3(LANES), 0, st, records, n, delta_words(depth), depth - 1u, totals);
}

void delta_apply_run(const uint2* records, uint32_t n, uint32_t* words, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(k_delta_apply, dim3((n + 255u) / 256u), dim3(256), 0, st, records, n, words);
}

}  // namespace vrc
