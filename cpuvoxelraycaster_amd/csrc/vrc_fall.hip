// vrc_fall.hip -- loose pieces fall as rigid bodies (include/vrc.h: vrc_fall_drops, vrc_fall_place).
//
// The pieces are the components of a labelling (vrc_components.hip: one uint32 id per KEY, the key 8 B + (z&1) 4 + (y&1) 2 +
// (x&1) being the voxel's bit index in the occupancy field), F the solid voxels of a second field.  With g the unit step of
// the direction and q(v) the number of cells between v and the face the pieces fall towards, the drops D_i are the greatest
// integers with, for every voxel v of piece i:  D_i <= q(v);  D_i = 0 where v lies in F;  D_i <= k - 1 for v + k g in F;
// D_i <= D_j + k - 1 for v + k g in another piece j;  D_i <= drop_limit.  Only the NEAREST non-empty voxel ahead of v
// matters: if it is of v's own piece, that voxel carries v's constraints (and tighter ones); if it is of F or of a piece j,
// everything farther ahead bounds D_i through it.
//
// The constraint pass, one launch per round, is a scan of every voxel column along the direction from the far face
// backwards that carries "the nearest non-empty voxel ahead: the wall / F / piece j, at distance k" and lowers D[i] with a
// 32-bit vector atomicMin; a lowered value raises the changed flag.  D starts at drop_limit, or at 0xffffffff ("no bound
// yet", skipped as a D_j and saturating in the sum) without one.
//   Why any schedule gives the same answer: every value ever written is the start value or the right side of a constraint
//   evaluated with upper bounds of the D_j, so by induction every value is an upper bound of the greatest solution; values
//   only decrease; and a round that lowers nothing has found every constraint satisfied, so its values ARE a solution, hence
//   the greatest one.  In-place relaxation in whatever order the hardware runs the lanes therefore ends at the unique
//   result, and a round may use values lowered earlier in the same round.  The bound of the loop: vrc_fall.h.
// Shape of the pass.  A column along z is every fourth key (8 (z/2) + 4 (z&1) = 4 z), the four columns of a brick row
// interleave to contiguous keys: there a WAVE takes 64 consecutive cells of one column, finds the nearest non-empty cell
// ahead of all 64 from two ballots with a bit scan, and carries the state from chunk to chunk; the four waves of a workgroup
// take the four interleaved columns.  Along x and y a LANE takes a column, and neighbouring lanes take the columns (low bit
// of the third axis, z) whose keys lie next to each other.  Where all the lanes of a wave that have something to lower name
// one piece -- a 512 x 512 slab under the wall -- the wave takes the minimum and issues one atomic; a bound that would not
// lower D[i] is dropped after a plain load.  The launch covers the union of the pieces' boxes, extended to the far face.
// No workgroup waits for another.  Every atomic is a 32- or 64-bit vector atomic at agent scope in plain HIP C++.
//
// Measured on an MI355X at 512^3 on the FastNoise terrain (tools/bench_edit.py --fall, profiles/edit/bench_fall.json; two
// bands and a grid of cuts leave 404 loose blocks of 1.9 M voxels over 5.6 M supported ones; device time by events, median
// of 5): the whole vrc_fall_drops call towards -y 0.57 ms in 2 rounds (largest drop 7), vrc_fall_place of all pieces
// 0.19 ms, next to 1.93 ms of vrc_volume_label_components and 0.20 ms of vrc_labels_select of the same labels in the same
// run -- a round, with the call's allocation, init pass and flag read-back shared out, costs 0.15 of the labelling.  The
// rounds have not been timed apart.
#include "vrc_fall.h"

#include "vrc_box_words.h"
#include "vrc_group.h"

namespace {

constexpr uint32_t NONE = VRC_NO_COMPONENT;
constexpr uint32_t UNBOUND = 0xffffffffu;
constexpr uint32_t GROUP = 256;

// the scratch block in front of D, in uint32 words
enum : uint32_t {
    B_CHANGED = 0,
    B_NOT_LO = 1,         // ~lo of the union box per axis (so that the zeroed block is the empty box), 3 words
    B_HI = 4,             // 3 words
    B_MOVED_PIECES = 7,
    B_MAX_DROP = 8,
    B_MOVED_VOXELS = 10,  // 64 bits, 8-byte aligned
    B_WORDS = 12
};

struct Scan {
    uint32_t n, S;                 // bricks and voxels per axis
    uint32_t axis, side;
    uint32_t q_end;                // cells scanned from the far face: q = 0 .. q_end - 1
    uint32_t a0, na, b0, nb;       // the columns: x/y scans: a = the other of x / y (a0, na even), b = z;  z scan: a = x, b = y (all even)
};

__device__ __forceinline__ uint32_t key_of(uint32_t n, uint32_t x, uint32_t y, uint32_t z)
{
    return 8u * (uint32_t)brick_of(n, x, y, z) + voxel_bit(x, y, z);
}

__device__ __forceinline__ uint32_t load_drop(const uint32_t* D, uint32_t i)
{
    return __hip_atomic_load(D + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The constraint of one voxel: of piece `id` (NONE: no voxel), in F or not, q cells from the far face, with the nearest
// non-empty cell ahead at pq (-1: the wall) of piece pj (NONE: the wall or F).  true: D[id] <= *bound.
__device__ __forceinline__ bool constraint(const uint32_t* D, uint32_t id, bool in_f, uint32_t q, int32_t pq, uint32_t pj, uint32_t* bound)
{
    if (id == NONE) return false;
    if (in_f) { *bound = 0u; return true; }
    if (pj == id) return false;
    const uint32_t gap = (uint32_t)((int32_t)q - pq) - 1u;              // empty cells between the two
    if (pj == NONE) { *bound = gap; return true; }
    const uint32_t dj = load_drop(D, pj);
    if (dj == UNBOUND) return false;
    const unsigned long long sum = (unsigned long long)dj + gap;
    if (sum >= UNBOUND) return false;
    *bound = (uint32_t)sum;
    return true;
}

// D[id] = min(D[id], bound) for the lanes with `has`; called by whole waves.  One atomic where all of them name one piece.
__device__ __forceinline__ void lower(uint32_t* D, uint32_t id, uint32_t bound, bool has, uint32_t* changed)
{
    if (has && load_drop(D, id) <= bound) has = false;
    const unsigned long long live = __ballot(has);
    if (!live) return;                                                  // wave-uniform
    const int leader = __ffsll((long long)live) - 1;
    const uint32_t lid = __shfl(id, leader);
    if (__ballot(has && id != lid) == 0ull) {
        const uint32_t least = wave_min(has ? bound : UNBOUND);
        if ((int)(threadIdx.x & 63u) == leader && atomicMin(&D[lid], least) > least) *changed = 1u;
    } else if (has) {
        if (atomicMin(&D[id], bound) > bound) *changed = 1u;
    }
}

__global__ __launch_bounds__(GROUP) void k_fall_init(uint32_t C, uint32_t start, const vrc_component* __restrict__ records, uint32_t* __restrict__ block,
                                                      uint32_t* __restrict__ D)
{
    const uint32_t i = blockIdx.x * GROUP + threadIdx.x;
    const bool live = i < C;
    if (live) D[i] = start;
    for (int a = 0; a < 3; ++a) {
        const uint32_t not_lo = wave_max(live ? ~records[i].lo[a] : 0u), hi = wave_max(live ? records[i].hi[a] : 0u);
        if ((threadIdx.x & 63u) == 0u) { atomicMax(&block[B_NOT_LO + a], not_lo); atomicMax(&block[B_HI + a], hi); }
    }
}

// scan along x or y: a lane per column
__global__ __launch_bounds__(GROUP) void k_fall_lanes(Scan s, const uint32_t* __restrict__ L, const uint32_t* __restrict__ F, uint32_t* D, uint32_t* changed)
{
    const uint32_t columns = s.na * s.nb;
    if (blockIdx.x * GROUP + (threadIdx.x & ~63u) >= columns) return;  // whole waves
    uint32_t c = blockIdx.x * GROUP + threadIdx.x;
    const bool live = c < columns;
    if (!live) c = 0u;
    uint32_t xyz[3];
    const uint32_t other = s.axis == 0u ? 1u : 0u;
    xyz[other] = s.a0 + 2u * ((c >> 1) / s.nb) + (c & 1u);
    xyz[2] = s.b0 + (c >> 1) % s.nb;
    int32_t pq = -1;
    uint32_t pj = NONE;
    for (uint32_t q = 0; q < s.q_end; ++q) {                            // uniform trip count
        xyz[s.axis] = s.side ? s.S - 1u - q : q;
        const uint32_t key = key_of(s.n, xyz[0], xyz[1], xyz[2]);
        const uint32_t id = live ? L[key] : NONE;
        const bool in_f = live && F && ((F[key >> 5] >> (key & 31u)) & 1u);
        uint32_t bound = 0u;
        const bool has = constraint(D, id, in_f, q, pq, pj, &bound);
        lower(D, id, bound, has, changed);
        if (in_f) { pq = (int32_t)q; pj = NONE; }
        else if (id != NONE) { pq = (int32_t)q; pj = id; }
    }
}

// scan along z: a wave per column, 64 cells at a time
__global__ __launch_bounds__(GROUP) void k_fall_wave(Scan s, const uint32_t* __restrict__ L, const uint32_t* __restrict__ F, uint32_t* D, uint32_t* changed)
{
    const uint32_t column = blockIdx.x * (GROUP / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (column >= s.na * s.nb) return;                                  // whole waves
    const uint32_t row = column >> 2, half = s.nb >> 1;
    const uint32_t x = s.a0 + 2u * (row / half) + (column & 1u), y = s.b0 + 2u * (row % half) + ((column >> 1) & 1u);
    int32_t carry_q = -1;
    uint32_t carry_j = NONE;
    for (uint32_t qb = 0; qb < s.q_end; qb += 64u) {                    // wave-uniform
        const uint32_t q = qb + lane;
        const bool live = q < s.q_end;
        const uint32_t z = live ? (s.side ? s.S - 1u - q : q) : 0u;
        const uint32_t key = key_of(s.n, x, y, z);
        const uint32_t id = live ? L[key] : NONE;
        const bool in_f = live && F && ((F[key >> 5] >> (key & 31u)) & 1u);
        const unsigned long long occupied = __ballot(id != NONE || in_f), fixed = __ballot(in_f);
        // the nearest non-empty cell ahead: the highest occupied lane below this one, or what the chunks before left
        const unsigned long long below = occupied & ((1ull << lane) - 1ull);
        const int near = below ? 63 - __clzll((long long)below) : 0;
        const uint32_t near_id = __shfl(id, near);
        int32_t pq = carry_q;
        uint32_t pj = carry_j;
        if (below) { pq = (int32_t)(qb + (uint32_t)near); pj = (fixed >> near) & 1ull ? NONE : near_id; }
        uint32_t bound = 0u;
        const bool has = constraint(D, id, in_f, q, pq, pj, &bound);
        lower(D, id, bound, has, changed);
        const int last = occupied ? 63 - __clzll((long long)occupied) : 0;
        const uint32_t last_id = __shfl(id, last);
        if (occupied) { carry_q = (int32_t)(qb + (uint32_t)last); carry_j = (fixed >> last) & 1ull ? NONE : last_id; }
    }
}

// offsets[3i + a] = D_i * g, and the stats from D and the records' voxel counts
__global__ __launch_bounds__(GROUP) void k_fall_finish(uint32_t C, uint32_t axis, int32_t sign, const vrc_component* __restrict__ records,
                                                        const uint32_t* __restrict__ D, int32_t* __restrict__ offsets, uint32_t* __restrict__ block)
{
    const uint32_t i = blockIdx.x * GROUP + threadIdx.x;
    const bool live = i < C;
    const uint32_t d = live ? D[i] : 0u;
    if (live)
        for (uint32_t a = 0; a < 3u; ++a) offsets[3u * i + a] = a == axis ? sign * (int32_t)d : 0;
    const unsigned long long moved = __ballot(d != 0u);
    if (!moved) return;                                                 // wave-uniform
    const unsigned long long voxels = wave_sum(d ? (unsigned long long)records[i].voxels : 0ull);
    const uint32_t most = wave_max(d);
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd((unsigned long long*)(block + B_MOVED_VOXELS), voxels);
        atomicAdd(&block[B_MOVED_PIECES], (uint32_t)__popcll(moved));
        atomicMax(&block[B_MAX_DROP], most);
    }
}

// A lane per key, as the select kernel: the lanes of a wave whose targets fall into one word of dst join their bits and
// issue one atomic, so a word is touched only where a bit is set and the result does not depend on the schedule.
__global__ __launch_bounds__(GROUP) void k_labels_place(uint32_t lg, uint32_t n_keys, const uint32_t* __restrict__ L, const uint8_t* __restrict__ keep,
                                                         const int32_t* __restrict__ offsets, uint32_t* dst, int op)
{
    const uint32_t key = blockIdx.x * GROUP + threadIdx.x;             // whole waves pass or fail the bound
    if (key >= n_keys) return;
    const uint32_t id = L[key];
    bool in = id != NONE && (!keep || keep[id] != 0);
    if (!__ballot(in)) return;                                          // a wave outside M: nothing more is loaded
    uint32_t word = 0u, bit = 0u;
    if (in) {
        const uint32_t B = key >> 3, nm = (1u << lg) - 1u, S = 2u << lg;
        const int32_t c[3] = {(int32_t)(2u * (B >> (2u * lg)) + (key & 1u)), (int32_t)(2u * ((B >> lg) & nm) + ((key >> 1) & 1u)),
                              (int32_t)(2u * (B & nm) + ((key >> 2) & 1u))};
        uint32_t t[3];
        for (int a = 0; a < 3; ++a) {
            const int32_t o = offsets[3u * id + a];
            if (o < -vrc::PLACE_OFFSET_LIMIT || o > vrc::PLACE_OFFSET_LIMIT) in = false;
            t[a] = (uint32_t)(c[a] + (in ? o : 0));                     // below 0 wraps to above S
            if (t[a] >= S) in = false;
        }
        if (in) {
            const uint32_t target = key_of(1u << lg, t[0], t[1], t[2]);
            word = target >> 5;
            bit = 1u << (target & 31u);
        }
    }
    unsigned long long todo = __ballot(in);
    while (todo) {                                                      // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lword = __shfl(word, leader);
        const bool mine = in && word == lword;
        todo &= ~__ballot(mine);
        uint32_t bits = mine ? bit : 0u;
        for (int o = 32; o; o >>= 1) bits |= __shfl_xor(bits, o);
        if ((int)(threadIdx.x & 63u) == leader) {
            if (op == VRC_COPY_OR) atomicOr(&dst[lword], bits);
            else atomicAnd(&dst[lword], ~bits);
        }
    }
}

}  // namespace

namespace vrc {

size_t fall_scratch_bytes(uint64_t pieces) { return ((size_t)B_WORDS + (size_t)pieces) * 4u; }

hipError_t fall_run(const uint32_t* labels, const vrc_component* records, uint64_t pieces, uint32_t depth, const uint32_t* fixed, int direction,
                    uint32_t drop_limit, int32_t* offsets, uint32_t* scratch, hipStream_t st, vrc_fall_stats* stats, uint32_t* converged)
{
    const uint32_t C = (uint32_t)pieces, S = 1u << depth;
    uint32_t* block = scratch;
    uint32_t* D = scratch + B_WORDS;
    const dim3 per_piece((C + GROUP - 1u) / GROUP), group(GROUP);
    uint32_t host[B_WORDS];
    *converged = 0u;
    hipError_t e = hipMemsetAsync(block, 0, B_WORDS * 4u, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fall_init, per_piece, group, 0, st, C, drop_limit ? drop_limit : UNBOUND, records, block, D);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(host, block, sizeof host, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;

    // the union of the pieces' boxes (every piece has a voxel: lo < hi <= S), extended to the far face
    uint32_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = ~host[B_NOT_LO + a]; hi[a] = host[B_HI + a];
        if (lo[a] >= hi[a] || hi[a] > S) return hipErrorInvalidValue;  // records that are not a labelling's: nothing is launched
    }
    Scan s;
    s.n = S >> 1; s.S = S;
    s.axis = fall_axis(direction); s.side = (uint32_t)direction & 1u;
    s.q_end = s.side ? S - lo[s.axis] : hi[s.axis];
    const uint32_t a = s.axis == 2u ? 0u : (s.axis == 0u ? 1u : 0u);   // the axis whose columns come in pairs
    s.a0 = lo[a] & ~1u; s.na = ((hi[a] + 1u) & ~1u) - s.a0;
    if (s.axis == 2u) { s.b0 = lo[1] & ~1u; s.nb = ((hi[1] + 1u) & ~1u) - s.b0; }
    else { s.b0 = lo[2]; s.nb = hi[2] - lo[2]; }
    const uint32_t columns = s.na * s.nb;                               // at most S^2 = 2^20
    const dim3 grid(s.axis == 2u ? (columns + GROUP / 64u - 1u) / (GROUP / 64u) : (columns + GROUP - 1u) / GROUP);

    uint32_t rounds = 0u;
    for (uint64_t r = 0; r < fall_round_bound(pieces) && !*converged; ++r) {
        uint32_t changed = 0u;
        if ((e = hipMemsetAsync(block + B_CHANGED, 0, 4u, st)) != hipSuccess) return e;
        if (s.axis == 2u) hipLaunchKernelGGL(k_fall_wave, grid, group, 0, st, s, labels, fixed, D, block + B_CHANGED);
        else hipLaunchKernelGGL(k_fall_lanes, grid, group, 0, st, s, labels, fixed, D, block + B_CHANGED);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(&changed, block + B_CHANGED, 4u, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
        ++rounds;
        if (!changed) *converged = 1u;
    }
    if (stats) stats->rounds = rounds;
    if (!*converged) return hipSuccess;

    hipLaunchKernelGGL(k_fall_finish, per_piece, group, 0, st, C, s.axis, fall_sign(direction), records, D, offsets, block);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(host, block, sizeof host, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (stats) {
        stats->moved_voxels = (uint64_t)host[B_MOVED_VOXELS] | (uint64_t)host[B_MOVED_VOXELS + 1u] << 32;
        stats->pieces = C; stats->moved_pieces = host[B_MOVED_PIECES];
        stats->max_drop = host[B_MAX_DROP];
        stats->reserved[0] = stats->reserved[1] = 0u;
    }
    return hipSuccess;
}

void place_run(const uint32_t* labels, uint32_t depth, const uint8_t* keep, const int32_t* offsets, uint32_t* dst, int op, hipStream_t st)
{
    const uint32_t n_keys = 1u << (3u * depth);
    hipLaunchKernelGGL(k_labels_place, dim3((n_keys + GROUP - 1u) / GROUP), dim3(GROUP), 0, st, depth - 1u, n_keys, labels, keep, offsets, dst, op);
}

}  // namespace vrc
