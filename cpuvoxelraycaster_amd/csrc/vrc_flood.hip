// vrc_flood.hip -- flood fill by connectivity on the editable volume's bit field (include/vrc.h: vrc_volume_flood).
//
// The occupancy is one byte per 2 x 2 x 2 brick, bit z*4 + y*2 + x, four bricks along z per 32-bit word: a word is
// 2 x 2 x 8 voxels and voxel (xb, yb, zz) of it, zz = 0..7, is bit zz*4 + yb*2 + xb -- eight z layers of one nibble.
// A one-voxel step is therefore a shift of the word: by 4 along z (the carry is a nibble of the z-neighbour word), by 1
// along x under the masks 0x5555.. / 0xAAAA.. (the carry comes from the word of the next brick in x), by 2 along y
// under 0x3333.. / 0xCCCC...  The flood iterates  region |= dilate(region) & M  on whole words; no voxel is ever
// expanded to a byte or a label.
//
// Work is cut into tiles of 32^3 voxels = 16 x 16 x 4 words, one 256-thread workgroup each, a thread owning the four
// words of one (x, y) column.  A sweep is one launch over all tiles:
//   * a tile runs only if it or one of its 26 neighbours changed in the sweep before (per-tile flags, three buffers in
//     rotation: read the last sweep's, write this sweep's, zero the next one's) -- every other workgroup leaves at once,
//     so the cost follows the frontier;
//   * it stages its region words and a one-word halo in LDS, iterates there until nothing changes or FLOOD_TILE_ITERS
//     is reached, writes back the words it changed, raises its flag and counts itself in the sweep's counter.
// There is no waiting between workgroups anywhere.  A halo word may be stale (the neighbour is writing it in the same
// sweep): the field only ever gains bits and every bit written is a bit of the answer, so a stale read costs a sweep,
// never a wrong bit.  Whole-word plain stores: a word has one owner.
#include "vrc_flood.h"

namespace {

constexpr uint32_t FLOOD_TILE_ITERS = 128;     // trip bound of the LDS loop; a tile that hits it changed, so it runs again
constexpr uint32_t FLOOD_BATCH_MAX = 8;        // sweeps between two reads of the counters
constexpr uint32_t TW = 16, TWZ = 4;           // words per tile along x / y, along z
constexpr uint32_t HX = TW + 2, HZ = TWZ + 2;  // with the halo
constexpr uint32_t HZP = HZ + 1;               // padded: neighbouring columns 7 words apart fall on different LDS banks

constexpr uint32_t X0 = vrc::WORD_X0, X1 = vrc::WORD_X1, Y0 = vrc::WORD_Y0, Y1 = vrc::WORD_Y1;

// w and what steps into it along x from itself and from the words of the bricks before (l) and after (r)
__device__ __forceinline__ uint32_t dilate_x(uint32_t w, uint32_t l, uint32_t r)
{
    return w | ((w & X0) << 1) | ((w & X1) >> 1) | ((l & X1) >> 1) | ((r & X0) << 1);
}
__device__ __forceinline__ uint32_t dilate_y(uint32_t w, uint32_t l, uint32_t r)
{
    return w | ((w & Y0) << 2) | ((w & Y1) >> 2) | ((l & Y1) >> 2) | ((r & Y0) << 2);
}
__device__ __forceinline__ uint32_t dilate_z(uint32_t w, uint32_t below, uint32_t above)
{
    return w | (w << 4) | (w >> 4) | (below >> 28) | (above << 28);
}

__device__ __forceinline__ uint32_t tiles_per_axis(uint32_t S) { return S >= 32u ? S >> 5 : 1u; }

// region &= M (seeds outside M are dropped BEFORE the first sweep, so that no halo ever shows a bit outside M), and the
// flags the first sweep reads: a tile with a region bit.  A tile without one, next to none, is at its fixed point.
__global__ void k_flood_prepare(uint32_t* region, const uint32_t* __restrict__ medium, uint32_t through, uint32_t n, uint32_t nwz,
                                uint64_t n_words, uint32_t* flags)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_words) return;
    const uint32_t m = through ? ~medium[i] : medium[i];
    const uint32_t have = region[i], r = have & m;
    if (r != have) region[i] = r;
    if (!r) return;
    const uint32_t wz = (uint32_t)(i % nwz), cy = (uint32_t)((i / nwz) % n), cx = (uint32_t)(i / ((uint64_t)nwz * n));
    const uint32_t T = tiles_per_axis(2u * n);
    flags[((cx / TW) * T + cy / TW) * T + wz / TWZ] = 1u;      // every writer writes the same value
}

// One sweep.  blockIdx.x = tile.  n = words per axis along x and y (bricks), nwz = words along z, T = tiles per axis.
// Words beyond the volume's faces read as region 0 and M 0: the faces are walls, also for the EMPTY flood.
template <int CONN>
__global__ __launch_bounds__(256) void k_flood_sweep(uint32_t* region, const uint32_t* __restrict__ medium, uint32_t through, uint32_t n,
                                                     uint32_t nwz, uint32_t T, const uint32_t* __restrict__ flags_prev, uint32_t* flags_now,
                                                     uint32_t* flags_next, uint32_t* counter)
{
    __shared__ uint32_t R[HX * HX * HZP];
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

    const int32_t ox = tx * (int32_t)TW - 1, oy = ty * (int32_t)TW - 1, oz = tz * (int32_t)TWZ - 1;
    for (uint32_t i = threadIdx.x; i < HX * HX * HZ; i += 256u) {
        const uint32_t lz = i % HZ, ly = (i / HZ) % HX, lx = i / (HZ * HX);
        const int32_t gx = ox + (int32_t)lx, gy = oy + (int32_t)ly, gz = oz + (int32_t)lz;
        uint32_t v = 0u;
        if (gx >= 0 && gy >= 0 && gz >= 0 && gx < (int32_t)n && gy < (int32_t)n && gz < (int32_t)nwz)
            v = region[((uint64_t)gx * n + (uint32_t)gy) * nwz + (uint32_t)gz];
        R[(lx * HX + ly) * HZP + lz] = v;
    }
    // this thread's column: words (cx, cy, cz0 .. cz0 + 3), at R[col + 1 .. col + 4]
    const uint32_t lx = threadIdx.x >> 4, ly = threadIdx.x & 15u;
    const uint32_t cx = (uint32_t)tx * TW + lx, cy = (uint32_t)ty * TW + ly, cz0 = (uint32_t)tz * TWZ;
    const uint32_t col = ((lx + 1u) * HX + (ly + 1u)) * HZP;
    const uint64_t g0 = ((uint64_t)cx * n + cy) * nwz + cz0;
    uint32_t m[TWZ], own[TWZ], first[TWZ];
    for (uint32_t k = 0; k < TWZ; ++k) {
        m[k] = 0u;
        if (cx < n && cy < n && cz0 + k < nwz) m[k] = through ? ~medium[g0 + k] : medium[g0 + k];
    }
    __syncthreads();
    for (uint32_t k = 0; k < TWZ; ++k) first[k] = own[k] = R[col + 1u + k];

    const uint32_t sx = HX * HZP, sy = HZP;     // LDS strides to the next column in x, in y
    // In the loop other threads read R while its owners write their words.  volatile: every read and write is a real,
    // whole 32-bit LDS access where it stands, never hoisted, merged or split.
    volatile uint32_t* Rv = R;
    for (uint32_t it = 0; it < FLOOD_TILE_ITERS; ++it) {
        uint32_t d[TWZ];
        if (CONN == 6) {
            for (uint32_t k = 0; k < TWZ; ++k) {
                const uint32_t a = col + 1u + k, w = own[k];
                d[k] = dilate_x(w, Rv[a - sx], Rv[a + sx]) | dilate_y(w, Rv[a - sy], Rv[a + sy]) | dilate_z(w, Rv[a - 1u], Rv[a + 1u]);
            }
        } else {
            // x, then y, then z: the three per-axis dilations compose to the 3 x 3 x 3 neighbourhood
            uint32_t yx[HZ];
            for (uint32_t k = 0; k < HZ; ++k) {
                const uint32_t a = col + k;
                const uint32_t lo = dilate_x(Rv[a - sy], Rv[a - sy - sx], Rv[a - sy + sx]);
                const uint32_t mid = dilate_x(Rv[a], Rv[a - sx], Rv[a + sx]);
                const uint32_t hi = dilate_x(Rv[a + sy], Rv[a + sy - sx], Rv[a + sy + sx]);
                yx[k] = dilate_y(mid, lo, hi);
            }
            for (uint32_t k = 0; k < TWZ; ++k) d[k] = dilate_z(yx[k + 1u], yx[k], yx[k + 2u]);
        }
        int changed = 0;
        for (uint32_t k = 0; k < TWZ; ++k) {
            const uint32_t w = own[k] | (d[k] & m[k]);
            if (w != own[k]) { own[k] = w; Rv[col + 1u + k] = w; changed = 1; }
        }
        // A reader sees a neighbour's word before or after its owner's write of this iteration, both subsets of the
        // answer.  The barrier ends the iteration; its result is uniform, so the loop is left by all threads together.
        if (!__syncthreads_or(changed)) break;
    }

    int wrote = 0;
    for (uint32_t k = 0; k < TWZ; ++k)
        if (own[k] != first[k]) { region[g0 + k] = own[k]; wrote = 1; }      // m[k] != 0 here: the word lies in the volume
    if (__syncthreads_or(wrote) && threadIdx.x == 0) {
        flags_now[tile] = 1u;
        atomicAdd(counter, 1u);
    }
}

// 4^3: two words, two brick rows to a word.  One workgroup, a thread per voxel, to the fixed point in one launch: an
// iteration before it adds a voxel, and there are 64.
template <int CONN>
__global__ __launch_bounds__(64) void k_flood_small(uint32_t* region, const uint32_t* __restrict__ medium, uint32_t through)
{
    __shared__ volatile uint32_t r[64];        // read by the neighbours while the owner writes it: whole accesses, never hoisted
    __shared__ uint32_t out[2];
    const uint32_t v = threadIdx.x, x = v >> 4, y = (v >> 2) & 3u, z = v & 3u;
    const uint32_t byte = (x >> 1) * 4u + (y >> 1) * 2u + (z >> 1);
    const uint32_t shift = 8u * (byte & 3u) + (z & 1u) * 4u + (y & 1u) * 2u + (x & 1u);
    const uint32_t med = (medium[byte >> 2] >> shift) & 1u;
    const uint32_t in_m = through ? med ^ 1u : med;
    uint32_t mine = (region[byte >> 2] >> shift) & in_m & 1u;
    r[v] = mine;
    if (v < 2u) out[v] = 0u;
    __syncthreads();
    for (uint32_t it = 0; it < 64u; ++it) {
        uint32_t any = 0u;
        for (int32_t dx = -1; dx <= 1; ++dx)
            for (int32_t dy = -1; dy <= 1; ++dy)
                for (int32_t dz = -1; dz <= 1; ++dz) {
                    if (CONN == 6 && (dx != 0) + (dy != 0) + (dz != 0) != 1) continue;
                    const int32_t nx = (int32_t)x + dx, ny = (int32_t)y + dy, nz = (int32_t)z + dz;
                    if (nx < 0 || ny < 0 || nz < 0 || nx > 3 || ny > 3 || nz > 3) continue;
                    any |= r[nx * 16 + ny * 4 + nz];
                }
        const int changed = !mine && in_m && any;
        if (changed) { mine = 1u; r[v] = 1u; }
        if (!__syncthreads_or(changed)) break;
    }
    if (mine) atomicOr(&out[byte >> 2], 1u << shift);
    __syncthreads();
    if (v < 2u) region[v] = out[v];
}

}  // namespace

namespace vrc {

size_t flood_scratch_bytes(uint32_t depth)
{
    const uint32_t S = 1u << depth, T = S >= 32u ? S >> 5 : 1u;
    return ((size_t)3u * T * T * T + FLOOD_BATCH_MAX) * 4u;
}

// Every sweep before the fixed point sets at least one voxel of M (a sweep that sets none has read the final state
// everywhere, see flood_run), and M has at most 8^depth voxels; one more sweep sees that nothing changes.
uint32_t flood_sweep_bound(uint32_t depth) { return (1u << (3u * depth)) + 1u; }

hipError_t flood_run(uint32_t* region, const uint32_t* medium, uint32_t depth, int connectivity, int through, uint32_t max_sweeps,
                     uint32_t* scratch, hipStream_t st, uint32_t* sweeps, uint32_t* converged)
{
    *sweeps = 0; *converged = 0;
    hipError_t e;
    if (depth == 2u) {
        if (connectivity == 6) hipLaunchKernelGGL(k_flood_small<6>, dim3(1), dim3(64), 0, st, region, medium, through ? 1u : 0u);
        else hipLaunchKernelGGL(k_flood_small<26>, dim3(1), dim3(64), 0, st, region, medium, through ? 1u : 0u);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        *sweeps = 1; *converged = 1;
        return hipStreamSynchronize(st);
    }
    const uint32_t S = 1u << depth, n = S >> 1, nwz = S >> 3, T = S >= 32u ? S >> 5 : 1u, tiles = T * T * T;
    const uint64_t n_words = (uint64_t)n * n * nwz;
    uint32_t* flags = scratch;
    uint32_t* counters = scratch + 3u * (size_t)tiles;
    if ((e = hipMemsetAsync(scratch, 0, flood_scratch_bytes(depth), st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_flood_prepare, dim3((uint32_t)((n_words + 255u) / 256u)), dim3(256), 0, st, region, medium, through ? 1u : 0u, n, nwz,
                       n_words, flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    // TERMINATION.  A tile that is skipped in sweep s (no flag of sweep s - 1 on it or around it) is at its local fixed
    // point: when it last ran it stopped changing against the halo it had loaded, and since then neither it nor a
    // neighbour has written a word, or a flag would stand.  (A tile that left its LDS loop at the trip bound wrote, so
    // it is flagged.)  So a sweep in which NO tile wrote a bit -- counter 0 -- leaves every tile at its local fixed
    // point against the final state of its neighbours, and a voxel's whole neighbourhood lies in its tile plus halo:
    // that is the global fixed point of  region |= dilate(region) & M.  It contains the seeds in M, and every bit ever
    // written was joined to one, so it is exactly the answer, whatever the schedule.  Sweeps after it are skipped by
    // every workgroup.  The counters of a batch are read together; the batches grow 2, 4, 8, 8, ...
    uint32_t issued = 0, batch = 2u;
    uint32_t host_counts[FLOOD_BATCH_MAX];
    for (;;) {
        const uint32_t b = batch < max_sweeps - issued ? batch : max_sweeps - issued;
        if (issued && (e = hipMemsetAsync(counters, 0, FLOOD_BATCH_MAX * 4u, st)) != hipSuccess) return e;
        for (uint32_t i = 0; i < b; ++i) {
            const uint32_t s = issued + 1u + i;          // sweep s reads buffer (s - 1) % 3, writes s % 3, zeroes (s + 1) % 3
            const uint32_t* prev = flags + (size_t)((s - 1u) % 3u) * tiles;
            uint32_t* now = flags + (size_t)(s % 3u) * tiles;
            uint32_t* next = flags + (size_t)((s + 1u) % 3u) * tiles;
            if (connectivity == 6)
                hipLaunchKernelGGL(k_flood_sweep<6>, dim3(tiles), dim3(256), 0, st, region, medium, through ? 1u : 0u, n, nwz, T, prev, now, next, counters + i);
            else
                hipLaunchKernelGGL(k_flood_sweep<26>, dim3(tiles), dim3(256), 0, st, region, medium, through ? 1u : 0u, n, nwz, T, prev, now, next, counters + i);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(host_counts, counters, b * 4u, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        issued += b;
        for (uint32_t i = 0; i < b; ++i)
            if (host_counts[i] == 0u) *converged = 1;
        if (*converged || issued == max_sweeps) break;
        if (batch < FLOOD_BATCH_MAX) batch *= 2u;
    }
    *sweeps = issued;
    return hipSuccess;
}

}  // namespace vrc
