// vrc_travel.hip -- the travel-distance field on the editable volume's bit field (include/vrc.h: vrc_travel_field)
// and the routes read off it (vrc_travel_trace_paths).
//
// T(p) = the least number of steps of a chain of neighbours lying in M from any seed to p, every step 1; the field is dense,
// [(x*S + y)*S + z], 32 bits a voxel, VRC_DISTANCE_NONE = "no value".  The occupancy layout (a word = 2 x 2 x 8 voxels) is
// described at the top of vrc_flood.hip, and the sweep scheme is the flood's:
//
//   init    k_travel_init: a thread per run of eight voxels along z writes 0 at seeds & M and NONE elsewhere, raises the
//           flag of a tile that holds a seed and counts the seeds (one 64-bit atomic per workgroup).
//   sweeps  k_travel_sweep: a launch over all tiles of 16^3 voxels, one 256-thread workgroup each, a thread owning one z
//           column of 16.  A tile runs only if it or one of its 26 neighbours changed in the sweep before (three per-tile
//           flag buffers in rotation: read the last sweep's, write this sweep's, zero the next one's).  It stages its values
//           with a one-voxel halo in LDS (18 x 18 x 19 words, 24 KiB: 32^3 with a halo would not fit a compute unit's LDS
//           next to a second workgroup), takes its M bits from the occupancy words, and iterates
//               T(p) = min(T(p), 1 + min over the neighbours q of T(q))        for p in M
//           until nothing changes or TRAVEL_TILE_ITERS is reached; the + 1 is only taken from a value below the limit (the
//           step limit, or NONE), so NONE never wraps and nothing at or beyond the limit propagates.  An iteration reads the
//           lateral neighbours from LDS and then runs up and down its own column in registers, so a value crosses the whole
//           column in one iteration.  The tile writes back the columns it lowered with plain stores (a voxel has one owner),
//           raises its flag and counts itself in the sweep's counter.
//   stats   k_travel_stats: the voxels with a value, and (max << 32) | ~dense index by a 64-bit vector atomicMax, monotone
//           in "larger value, then smaller index" (the distance transform's packed slot).
//
// No workgroup waits for another.  The host ends the loop when a sweep's counter is 0; the counters are read in batches.
//
// WHY THE RESULT IS T, WHATEVER THE SCHEDULE
//   (1) Every value ever written is the length of a real chain in M from a seed: the init pass writes 0 at seeds in M, and a
//       voxel of M only ever takes v(q) + 1 from a neighbour q whose value was a chain's length when it was read.  So every
//       value is an upper bound on T, and a voxel outside M keeps NONE for ever (its M bit is never set): only p's own
//       M bit has to be tested, a neighbour outside M can never lend a value.
//   (2) Values only decrease (a store happens only for a smaller value; the owner is the only writer), so a stale read -- a
//       halo word the neighbouring tile is lowering in the same sweep, an LDS word its owner is lowering in the same
//       iteration -- is a larger or equal value: still a real chain's length.  It can cost a sweep, never a wrong value.
//       Values are whole 32-bit words, read and written whole.
//   (3) After sweep k every voxel with T <= k holds T.  k = 0: the init pass.  Step: let T(p) = k + 1 and q a neighbour of p
//       with T(q) = k.  q took its final value in a sweep j <= k (or in the init pass, j = 0), which flagged q's tile (the
//       init pass flags the seeds' tiles); p's tile is that tile or one of its 26 neighbours, so it runs in sweep
//       j + 1 <= k + 1, stages q's final value -- a kernel boundary lies between -- and its first iteration gives p the value
//       k + 1, which (1) says is not too small.  A tile that is skipped has, like the flood's, nothing new around it.
//   (4) So sweep max T is the last that can change anything, sweep max T + 1 counts 0, and the host's loop bound
//       max T + 2 <= 8^depth + 1 is never reached; with a step limit L no value above L is ever stored, and the bound is
//       L + 2.  Reaching the bound is an internal error, not a partial result.
//   (5) A tile that left its LDS loop at the trip bound has lowered a value, so it is flagged and runs again; a sweep in
//       which no tile lowered a value (counter 0) leaves every tile at its local fixed point against the final state of its
//       neighbours, which is the global fixed point of the iteration, and by (1) and (3) that is T.
//
// Scratch: 24 bytes of stats, three flag words per tile and the counters -- 3 MiB at 1024^3 -- freed before the call returns.
// Measured on an MI355X at 512^3 on the FastNoise terrain (tools/bench_edit.py --travel, profiles/edit/bench_travel.json; device
// time by events, median of 5, vrc_volume_flood from the same seeds in the same run):
//   through the air from one seed, 58.3 M voxels:   6 neighbours 6.2 ms, 54 sweeps, 742 steps at most (flood 1.5 ms, 30 sweeps)
//                                                   26 neighbours 9.5 ms, 46 sweeps, 264 steps at most (flood 1.4 ms, 14 sweeps)
//   through the solid from the slab the terrain stands on, 8.6 M voxels, 78 steps at most:
//                                                   6 neighbours 1.05 ms, 26 neighbours 1.43 ms, 6 sweeps (flood 0.26 / 0.36 ms, 6 sweeps)
// The field moves 32 bits a voxel where the flood moves one, and the sweeps are far fewer than the steps: a sweep carries
// the frontier across a tile.
#include "vrc_travel.h"

#include "vrc_group.h"
#include "vrc_word_columns.h"

namespace {

constexpr uint32_t NONE = VRC_DISTANCE_NONE;
constexpr uint32_t TRAVEL_TILE_ITERS = 64;     // trip bound of the LDS loop; a tile that hits it changed, so it runs again
constexpr uint32_t TRAVEL_BATCH_MAX = 8;       // sweeps between two reads of the counters
constexpr uint32_t TV = 16;                    // voxels per tile along an axis
constexpr uint32_t HV = TV + 2;                // with the halo
constexpr uint32_t HZP = HV + 1;               // padded: neighbouring columns 19 words apart spread over the LDS banks
constexpr uint32_t GROUP = 256;

__host__ __device__ inline uint32_t tiles_per_axis(uint32_t S) { return S >= TV ? S / TV : 1u; }

// Bit k = voxel (x, y, 8*zseg + k) of the brick field `words` (n bricks per axis), XORed with `flip` (0 or ~0) inside the
// volume; 0 for everything outside it.  From 8^3 on a run of eight voxels along z is one aligned word; 4^3 (two brick rows to
// a word) reads its two bytes.
__device__ __forceinline__ uint32_t column_bits(const uint32_t* __restrict__ words, uint32_t n, uint32_t flip, uint32_t x, uint32_t y, uint32_t zseg)
{
    const uint32_t S = 2u * n;
    if (x >= S || y >= S || 8u * zseg >= S) return 0u;
    const uint32_t sh = (y & 1u) * 2u + (x & 1u);
    const uint32_t row = ((x >> 1) * n + (y >> 1)) * n;          // byte index of brick (x/2, y/2, 0): below 2^27
    if (n >= 4u) return (column_bits_of_word(words[(row >> 2) + zseg], sh) ^ flip) & 0xffu;
    const uint8_t* b = (const uint8_t*)words + row;
    uint32_t bits = 0u;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t v = (uint32_t)b[j] >> sh;
        bits |= ((v & 1u) | ((v >> 3) & 2u)) << (2u * j);
    }
    return (bits ^ flip) & ((1u << S) - 1u);
}

// A thread per run of eight voxels along z (of four at 4^3), z runs fastest over the threads: field = 0 at seeds & M, NONE
// elsewhere.  segs = runs per column, flags = the buffer sweep 1 reads.
__global__ __launch_bounds__(GROUP) void k_travel_init(const uint32_t* __restrict__ seeds, const uint32_t* __restrict__ medium, uint32_t flip, uint32_t depth,
                                                       uint32_t segs, uint32_t* __restrict__ field, uint32_t* flags, unsigned long long* stats)
{
    __shared__ uint32_t part[GROUP / 64u];
    const uint32_t S = 1u << depth, n = S >> 1;
    const uint64_t i = (uint64_t)blockIdx.x * GROUP + threadIdx.x, total = (uint64_t)S * S * segs;
    uint32_t s = 0u;
    if (i < total) {
        const uint32_t zseg = (uint32_t)(i % segs), y = (uint32_t)((i / segs) & (S - 1u)), x = (uint32_t)(i / ((uint64_t)segs * S));
        s = column_bits(seeds, n, 0u, x, y, zseg) & column_bits(medium, n, flip, x, y, zseg);
        uint32_t* run = field + ((((size_t)x << depth) | y) << depth) + 8u * zseg;
        uint32_t v[8];
        for (uint32_t k = 0; k < 8u; ++k) v[k] = (s >> k) & 1u ? 0u : NONE;
        *(uint4*)run = make_uint4(v[0], v[1], v[2], v[3]);
        if (S >= 8u) *(uint4*)(run + 4) = make_uint4(v[4], v[5], v[6], v[7]);
        if (s) {
            const uint32_t T = tiles_per_axis(S);
            flags[((x / TV) * T + y / TV) * T + (8u * zseg) / TV] = 1u;      // every writer writes the same value
        }
    }
    const uint32_t sum = group_sum<GROUP / 64u>(__popc(s), part);
    if (threadIdx.x == 0 && sum) atomicAdd(&stats[0], (unsigned long long)sum);
}

__device__ __forceinline__ uint32_t min4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

// One sweep.  blockIdx.x = tile, T = tiles per axis, limit = the step limit or NONE: a value below it may be stepped from.
// Voxels beyond the volume's faces read as NONE and are not in M: the faces are walls, also through the empty voxels.
template <int CONN>
__global__ __launch_bounds__(GROUP) void k_travel_sweep(uint32_t* field, const uint32_t* __restrict__ medium, uint32_t flip, uint32_t depth, uint32_t T,
                                                        uint32_t limit, const uint32_t* __restrict__ flags_prev, uint32_t* flags_now, uint32_t* flags_next,
                                                        uint32_t* counter)
{
    __shared__ uint32_t V[HV * HV * HZP];
    const uint32_t tile = blockIdx.x;
    const int32_t tz = (int32_t)(tile % T), ty = (int32_t)((tile / T) % T), tx = (int32_t)(tile / (T * T));
    if (threadIdx.x == 0) flags_next[tile] = 0u;
    int active = 0;
    if (threadIdx.x < 27u) {
        const int32_t ax = tx + (int32_t)(threadIdx.x / 9u) - 1, ay = ty + (int32_t)((threadIdx.x / 3u) % 3u) - 1, az = tz + (int32_t)(threadIdx.x % 3u) - 1;
        if (ax >= 0 && ay >= 0 && az >= 0 && ax < (int32_t)T && ay < (int32_t)T && az < (int32_t)T)
            active = (int)flags_prev[((uint32_t)ax * T + (uint32_t)ay) * T + (uint32_t)az];
    }
    if (!__syncthreads_or(active)) return;

    const int32_t S = (int32_t)(1u << depth);
    const int32_t ox = tx * (int32_t)TV - 1, oy = ty * (int32_t)TV - 1, oz = tz * (int32_t)TV - 1;
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < HV * HV * HV; i += GROUP) {
        const uint32_t lz = i % HV, ly = (i / HV) % HV, lx = i / (HV * HV);
        const int32_t gx = ox + (int32_t)lx, gy = oy + (int32_t)ly, gz = oz + (int32_t)lz;
        uint32_t v = NONE;
        if (gx >= 0 && gy >= 0 && gz >= 0 && gx < S && gy < S && gz < S) v = field[((((size_t)gx << depth) | (uint32_t)gy) << depth) | (uint32_t)gz];
        V[(lx * HV + ly) * HZP + lz] = v;
    }
    // this thread's column: voxels (x, y, z0 .. z0 + 15) at V[col + 1 .. col + 16], the halo below and above at col and col + 17
    const uint32_t lx = threadIdx.x >> 4, ly = threadIdx.x & 15u;
    const uint32_t x = (uint32_t)tx * TV + lx, y = (uint32_t)ty * TV + ly, z0 = (uint32_t)tz * TV;
    const uint32_t col = ((lx + 1u) * HV + (ly + 1u)) * HZP;
    const uint32_t n = (uint32_t)S >> 1;
    const uint32_t in_m = column_bits(medium, n, flip, x, y, z0 >> 3) | (column_bits(medium, n, flip, x, y, (z0 >> 3) + 1u) << 8);   // 0 outside the volume
    __syncthreads();
    uint32_t v[HV];
    for (uint32_t k = 0; k < HV; ++k) v[k] = V[col + k];

    const uint32_t sx = HV * HZP, sy = HZP;     // LDS strides to the next column in x, in y
    // In the loop other threads read V while its owners write their words: relaxed workgroup-scope atomic accesses, each a
    // real, whole 32-bit LDS access where it stands (ds_read_b32 / ds_write_b32), never hoisted out of the loop, merged or split.
    const auto Vv = [](uint32_t i) { return __hip_atomic_load(&V[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    uint32_t ever = 0u;                         // bit k: voxel z0 + k was lowered
#pragma unroll 1
    for (uint32_t it = 0; it < TRAVEL_TILE_ITERS; ++it) {
        uint32_t c[HV];                         // c[k], k = 1 .. 16: the least value around voxel k outside its own column
        if (CONN == 6) {
#pragma unroll
            for (uint32_t k = 1; k <= TV; ++k) {
                const uint32_t a = col + k;
                c[k] = min4(Vv(a - sx), Vv(a + sx), Vv(a - sy), Vv(a + sy));
            }
        } else {
            uint32_t ring[HV];                  // the least value of the eight columns around, layer by layer
#pragma unroll
            for (uint32_t k = 0; k < HV; ++k) {
                const uint32_t a = col + k;
                const uint32_t lo = min4(Vv(a - sx - sy), Vv(a - sx), Vv(a - sx + sy), Vv(a - sy));
                const uint32_t hi = min4(Vv(a + sx - sy), Vv(a + sx), Vv(a + sx + sy), Vv(a + sy));
                ring[k] = lo < hi ? lo : hi;
            }
#pragma unroll
            for (uint32_t k = 1; k <= TV; ++k) {
                const uint32_t m = ring[k - 1u] < ring[k + 1u] ? ring[k - 1u] : ring[k + 1u];
                c[k] = m < ring[k] ? m : ring[k];
            }
        }
        // up the column, then down: the voxel below / above is a neighbour under both connectivities
        uint32_t changed = 0u;
#pragma unroll
        for (uint32_t k = 1; k <= TV; ++k) {
            const uint32_t from = c[k] < v[k - 1u] ? c[k] : v[k - 1u];
            if (((in_m >> (k - 1u)) & 1u) && from < limit && from + 1u < v[k]) { v[k] = from + 1u; changed |= 1u << (k - 1u); }
        }
#pragma unroll
        for (uint32_t k = TV; k >= 1u; --k) {
            const uint32_t from = v[k + 1u];
            if (((in_m >> (k - 1u)) & 1u) && from < limit && from + 1u < v[k]) { v[k] = from + 1u; changed |= 1u << (k - 1u); }
        }
#pragma unroll
        for (uint32_t k = 1; k <= TV; ++k)
            if ((changed >> (k - 1u)) & 1u) __hip_atomic_store(&V[col + k], v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        ever |= changed;
        // A reader sees a neighbour's word before or after its owner's write of this iteration, both lengths of real chains.
        // The barrier ends the iteration; its result is uniform, so the loop is left by all threads together.
        if (!__syncthreads_or((int)changed)) break;
    }

    // in_m is 0 outside the volume, so a lowered voxel lies inside it, and with it the aligned run of four around it
    uint32_t* mine = field + ((((size_t)x << depth) | y) << depth) + z0;
#pragma unroll
    for (uint32_t q = 0; q < TV / 4u; ++q)
        if ((ever >> (4u * q)) & 15u) *(uint4*)(mine + 4u * q) = make_uint4(v[4u * q + 1u], v[4u * q + 2u], v[4u * q + 3u], v[4u * q + 4u]);
    if (__syncthreads_or((int)ever) && threadIdx.x == 0) {
        flags_now[tile] = 1u;
        atomicAdd(counter, 1u);
    }
}

// A thread per four voxels by grid stride: the voxels with a value, and the largest value with the smallest index that holds it.
__global__ __launch_bounds__(GROUP) void k_travel_stats(const uint32_t* __restrict__ field, uint32_t quads, unsigned long long* stats)
{
    __shared__ uint32_t part[GROUP / 64u];
    __shared__ unsigned long long red[GROUP];
    uint32_t reached = 0u;                      // at most 4 x 2^28 / gridDim per thread: fits
    unsigned long long best = 0ull;
    for (uint32_t qi = blockIdx.x * GROUP + threadIdx.x; qi < quads; qi += gridDim.x * GROUP) {
        const uint4 f = ((const uint4*)field)[qi];
        const uint32_t val[4] = {f.x, f.y, f.z, f.w};
        for (uint32_t k = 0; k < 4u; ++k) {
            if (val[k] == NONE) continue;
            ++reached;
            const unsigned long long packed = ((unsigned long long)val[k] << 32) | (uint32_t)~(4u * qi + k);
            best = packed > best ? packed : best;
        }
    }
    red[threadIdx.x] = best;
    __syncthreads();
    for (uint32_t s = GROUP / 2u; s; s >>= 1) {
        if (threadIdx.x < s && red[threadIdx.x + s] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + s];
        __syncthreads();
    }
    const uint32_t sum = group_sum<GROUP / 64u>(reached, part);
    if (threadIdx.x == 0 && sum) {
        atomicAdd(&stats[1], (unsigned long long)sum);
        atomicMax(&stats[2], red[0]);
    }
}

// One thread per route: not the hot path.  Nothing beyond the voxels written is touched.
__global__ void k_travel_trace(const uint32_t* __restrict__ field, uint32_t depth, int connectivity, uint64_t count, const uint32_t* __restrict__ start_xyz,
                               uint32_t capacity, uint32_t* __restrict__ paths, uint32_t* __restrict__ lengths)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t S = 1u << depth;
    uint32_t p[3] = {start_xyz[3 * i], start_xyz[3 * i + 1], start_xyz[3 * i + 2]};
    const uint32_t t = p[0] < S && p[1] < S && p[2] < S ? field[((((size_t)p[0] << depth) | p[1]) << depth) | p[2]] : NONE;
    lengths[i] = t;
    if (t == NONE || capacity == 0u) return;
    const uint32_t last = t < capacity - 1u ? t : capacity - 1u;
    uint32_t* row = paths + i * capacity * 3u;
    for (uint32_t k = 0;; ++k) {
        row[3 * (uint64_t)k] = p[0]; row[3 * (uint64_t)k + 1] = p[1]; row[3 * (uint64_t)k + 2] = p[2];
        if (k == last) break;
        const uint32_t want = t - k - 1u;
        bool found = false;
        for (int32_t d = 0; d < 27 && !found; ++d) {           // ascending (dx, dy, dz), dx most significant
            const int32_t dx = d / 9 - 1, dy = (d / 3) % 3 - 1, dz = d % 3 - 1;
            if (connectivity == VRC_CONNECT_FACES ? (dx != 0) + (dy != 0) + (dz != 0) != 1 : d == 13) continue;
            const uint32_t qx = p[0] + (uint32_t)dx, qy = p[1] + (uint32_t)dy, qz = p[2] + (uint32_t)dz;      // -1 wraps beyond S
            if (qx >= S || qy >= S || qz >= S) continue;
            if (field[((((size_t)qx << depth) | qy) << depth) | qz] != want) continue;
            p[0] = qx; p[1] = qy; p[2] = qz;
            found = true;
        }
        if (!found) break;       // not a travel field's: every voxel with a value t > 0 has a neighbour with t - 1
    }
}

}  // namespace

namespace vrc {

size_t travel_scratch_bytes(uint32_t depth)
{
    const uint32_t T = tiles_per_axis(1u << depth);
    return 24u + ((size_t)3u * T * T * T + TRAVEL_BATCH_MAX) * 4u;
}

unsigned long long* travel_stats_slots(uint32_t* scratch) { return (unsigned long long*)scratch; }

uint32_t travel_sweep_bound(uint32_t depth, uint32_t step_limit)
{
    const uint32_t whole = (1u << (3u * depth)) + 1u;
    return step_limit && step_limit < whole - 2u ? step_limit + 2u : whole;
}

hipError_t travel_run(const uint32_t* seeds, const uint32_t* medium, uint32_t depth, int connectivity, int through, uint32_t step_limit,
                      uint32_t* field, uint32_t* scratch, hipStream_t st, uint32_t* sweeps, uint32_t* converged)
{
    *sweeps = 0; *converged = 0;
    const uint32_t S = 1u << depth, T = tiles_per_axis(S), tiles = T * T * T, segs = S >= 8u ? S >> 3 : 1u;
    const uint32_t flip = through ? 0xffffffffu : 0u, limit = step_limit ? step_limit : NONE;
    unsigned long long* stats = travel_stats_slots(scratch);
    uint32_t* flags = scratch + 6;
    uint32_t* counters = flags + 3u * (size_t)tiles;
    hipError_t e;
    if ((e = hipMemsetAsync(scratch, 0, travel_scratch_bytes(depth), st)) != hipSuccess) return e;
    const uint64_t runs = (uint64_t)S * S * segs;
    hipLaunchKernelGGL(k_travel_init, dim3((uint32_t)((runs + GROUP - 1u) / GROUP)), dim3(GROUP), 0, st, seeds, medium, flip, depth, segs, field, flags, stats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    unsigned long long n_seeds = 0ull;
    if ((e = hipMemcpyAsync(&n_seeds, stats, 8, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (!n_seeds) {                // the field is all NONE and the stats slots are zero: no sweep, no stats pass
        *converged = 1;
        return hipSuccess;
    }

    // The loop of flood_run: the counters of a batch are read together; the batches grow 2, 4, 8, 8, ...  Sweeps issued
    // after the one that counted 0 are skipped by every workgroup.
    const uint32_t max_sweeps = travel_sweep_bound(depth, step_limit);
    uint32_t issued = 0, batch = 2u;
    uint32_t host_counts[TRAVEL_BATCH_MAX];
    for (;;) {
        const uint32_t b = batch < max_sweeps - issued ? batch : max_sweeps - issued;
        if (issued && (e = hipMemsetAsync(counters, 0, TRAVEL_BATCH_MAX * 4u, st)) != hipSuccess) return e;
        for (uint32_t i = 0; i < b; ++i) {
            const uint32_t s = issued + 1u + i;          // sweep s reads buffer (s - 1) % 3, writes s % 3, zeroes (s + 1) % 3
            const uint32_t* prev = flags + (size_t)((s - 1u) % 3u) * tiles;
            uint32_t* now = flags + (size_t)(s % 3u) * tiles;
            uint32_t* next = flags + (size_t)((s + 1u) % 3u) * tiles;
            if (connectivity == VRC_CONNECT_FACES)
                hipLaunchKernelGGL(k_travel_sweep<6>, dim3(tiles), dim3(GROUP), 0, st, field, medium, flip, depth, T, limit, prev, now, next, counters + i);
            else
                hipLaunchKernelGGL(k_travel_sweep<26>, dim3(tiles), dim3(GROUP), 0, st, field, medium, flip, depth, T, limit, prev, now, next, counters + i);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(host_counts, counters, b * 4u, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        issued += b;
        for (uint32_t i = 0; i < b; ++i)
            if (host_counts[i] == 0u) *converged = 1;
        if (*converged || issued == max_sweeps) break;
        if (batch < TRAVEL_BATCH_MAX) batch *= 2u;
    }
    *sweeps = issued;
    if (!*converged) return hipSuccess;

    const uint32_t quads = 1u << (3u * depth - 2u);
    const uint32_t want = (quads + GROUP - 1u) / GROUP;
    hipLaunchKernelGGL(k_travel_stats, dim3(want < 4096u ? want : 4096u), dim3(GROUP), 0, st, field, quads, stats);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipStreamSynchronize(st);
}

void travel_trace_run(const uint32_t* field, uint32_t depth, int connectivity, uint64_t n, const uint32_t* start_xyz, uint32_t capacity,
                      uint32_t* paths_xyz, uint32_t* lengths, hipStream_t st)
{
    hipLaunchKernelGGL(k_travel_trace, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, field, depth, connectivity, n, start_xyz, capacity, paths_xyz,
                       lengths);
}

}  // namespace vrc
