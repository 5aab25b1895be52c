// vrc_components.hip -- connected-component labelling of the editable volume's bit field (include/vrc.h:
// vrc_volume_label_components, vrc_labels_*).
//
// The occupancy is one byte per 2 x 2 x 2 brick, bit z*4 + y*2 + x, four bricks to a 32-bit word (the layout: top of
// vrc_flood.hip), so a voxel's KEY  8 B + (z&1) 4 + (y&1) 2 + (x&1)  is simply its bit index in the field: word key / 32,
// bit key % 32, at every depth, the two-word 4^3 volume included.  The labels are one uint32 per key, and a lane owns one
// key: 64 consecutive keys are two words, so label traffic is coalesced and a word's bits are a wave ballot.
//
// Union-find on the label array, every phase a kernel on one stream; no workgroup ever waits for another:
//   1. init     L[key] = key for the voxels of M, VRC_NO_COMPONENT elsewhere;
//   2. merge    a voxel of M unites itself with its neighbours of M in the earlier half of the neighbourhood (offsets that
//               are lexicographically negative: 3 of 6, 13 of 26; beyond the volume's faces there is no neighbour) -- with
//               a dense cell field (vrc_fracture_label), only with those that carry its own cell value.  find
//               follows parents and points every node it passes at its grandparent, union hooks the larger root under the
//               smaller with atomicMin and carries on with what the atomic returned where the node was a root no longer.
//               A parent is always a smaller key and a label is only ever lowered, so every loop ends on its own, and a
//               link that is replaced is re-united by the thread that replaced it: at the end of the kernel two voxels
//               are in one tree iff a chain of neighbours joins them.  The root of a tree is its smallest key;
//   3. flatten  L[key] = find(key), and the roots (L[key] == key) are counted per workgroup;
//   4. scan     one workgroup turns the counts into their exclusive prefix, the total C goes behind them (the host reads
//               it and makes room for the records);
//   5. roots    a root's rank in key order is its id: its record is started (first = the key decoded, an empty box) and
//               L[root] = id | ROOT_FLAG -- a key and an id are both below 2^30, the flag tells them apart;
//   6. ids      every other voxel of M takes its root's id; one pass adds voxel counts (64-bit) and boxes (min / max) to
//               the records, a wave first summing the lanes that share an id, so that a piece of millions of voxels costs
//               one set of atomics per wave and not per voxel;
//   7. strip    the roots drop the flag.
// Every atomic is a 32- or 64-bit vector atomic at agent scope in plain HIP C++.
#include "vrc_components.h"

#include "vrc_box_words.h"
#include "vrc_group.h"

namespace {

constexpr uint32_t NONE = VRC_NO_COMPONENT;
constexpr uint32_t ROOT_FLAG = 0x80000000u;
constexpr uint32_t GROUP = 256;               // lanes per workgroup
constexpr uint32_t ROUNDS = 32;               // a workgroup takes ROUNDS x GROUP consecutive keys (256 words)
constexpr uint32_t GROUP_KEYS = GROUP * ROUNDS;

struct Field {
    uint32_t lg;                              // log2 of the bricks per axis, n = S / 2
    uint32_t S;
    uint32_t n_keys;                          // 8^depth <= 2^30
    uint32_t flip;                            // ~0: M is the complement of the words (through the empty voxels)
};

__device__ __forceinline__ uint32_t key_of(const Field& f, uint32_t x, uint32_t y, uint32_t z) { return voxel_key(f.lg, x, y, z); }
__device__ __forceinline__ void voxel_of(const Field& f, uint32_t key, uint32_t c[3]) { key_voxel(f.lg, key, c); }

__device__ __forceinline__ uint32_t load_label(const uint32_t* L, uint32_t a)
{
    return __hip_atomic_load(L + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above a; every node passed is pointed at its grandparent (a label is only ever lowered)
__device__ __forceinline__ uint32_t find_and_shorten(uint32_t* L, uint32_t a)
{
    uint32_t p = load_label(L, a);
    while (p != a) {
        const uint32_t gp = load_label(L, p);
        if (gp != p) atomicMin(&L[a], gp);
        a = p;
        p = gp;
    }
    return a;
}

__device__ __forceinline__ void unite(uint32_t* L, uint32_t a, uint32_t b)
{
    a = find_and_shorten(L, a);
    b = find_and_shorten(L, b);
    while (a != b) {
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&L[a], b);      // a was a root iff old == a: then it hangs under b now
        if (old == a) break;
        a = old;                                       // a's parent of a moment ago: still to be joined with b
    }
}

__global__ __launch_bounds__(GROUP) void k_components_init(Field f, const uint32_t* __restrict__ words, uint32_t* __restrict__ L)
{
    for (uint32_t r = 0; r < ROUNDS; ++r) {
        const uint32_t key = blockIdx.x * GROUP_KEYS + r * GROUP + threadIdx.x;
        if (key >= f.n_keys) return;
        const uint32_t w = words[key >> 5] ^ f.flip;
        L[key] = (w >> (key & 31u)) & 1u ? key : NONE;
    }
}

// CELLS: the voxels also carry a cell value, cells[(x*S + y)*S + z] (vrc_fracture.hip), and only neighbours of one cell unite
template <int CONN, bool CELLS>
__global__ __launch_bounds__(GROUP) void k_components_merge(Field f, const uint32_t* __restrict__ words, uint32_t* L, const uint32_t* __restrict__ cells)
{
    for (uint32_t r = 0; r < ROUNDS; ++r) {
        const uint32_t key = blockIdx.x * GROUP_KEYS + r * GROUP + threadIdx.x;
        if (key >= f.n_keys) return;
        const uint32_t w = words[key >> 5] ^ f.flip;
        if (!((w >> (key & 31u)) & 1u)) continue;
        uint32_t c[3];
        voxel_of(f, key, c);
        const uint32_t dsh = f.lg + 1u;                                        // log2 S
        uint32_t mine = 0u;
        if (CELLS) mine = cells[(((size_t)c[0] << dsh | c[1]) << dsh) | c[2]];
#pragma unroll
        for (int dx = -1; dx <= 0; ++dx)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz) {
                    // the earlier half: (dx, dy, dz) < (0, 0, 0) in lexicographic order
                    if (!(dx < 0 || (dx == 0 && (dy < 0 || (dy == 0 && dz < 0))))) continue;
                    if (CONN == 6 && (dx != 0) + (dy != 0) + (dz != 0) != 1) continue;
                    const uint32_t x = c[0] + (uint32_t)dx, y = c[1] + (uint32_t)dy, z = c[2] + (uint32_t)dz;
                    if (x >= f.S || y >= f.S || z >= f.S) continue;        // below 0 wraps to above S
                    const uint32_t other = key_of(f, x, y, z);
                    const uint32_t ow = (other >> 5) == (key >> 5) ? w : words[other >> 5] ^ f.flip;
                    if (!((ow >> (other & 31u)) & 1u)) continue;
                    if (CELLS && cells[(((size_t)x << dsh | y) << dsh) | z] != mine) continue;
                    unite(L, key, other);
                }
    }
}

// No hook runs any more: the trees are final, and a thread that reads a label another thread has just flattened reads a
// node of the same path.
__global__ __launch_bounds__(GROUP) void k_components_flatten(Field f, uint32_t* L, uint32_t* __restrict__ slots)
{
    __shared__ uint32_t part[4];
    uint32_t roots = 0u;
    for (uint32_t r = 0; r < ROUNDS; ++r) {
        const uint32_t key = blockIdx.x * GROUP_KEYS + r * GROUP + threadIdx.x;
        if (key >= f.n_keys) break;
        uint32_t a = load_label(L, key);
        if (a == NONE) continue;
        if (a == key) { ++roots; continue; }
        for (uint32_t p = load_label(L, a); p != a; p = load_label(L, a)) a = p;
        L[key] = a;
    }
    const uint32_t s = group_sum<GROUP / 64u>(roots, part);
    if (threadIdx.x == 0) slots[blockIdx.x] = s;
}

__global__ __launch_bounds__(GROUP) void k_components_roots(Field f, uint32_t* L, const uint32_t* __restrict__ slots, vrc_component* __restrict__ records)
{
    __shared__ uint32_t part[4];
    uint32_t next = slots[blockIdx.x];
    if (next == slots[blockIdx.x + 1u]) return;                        // uniform for the workgroup
    for (uint32_t r = 0; r < ROUNDS; ++r) {                            // uniform trip count: the scan has barriers
        const uint32_t key = blockIdx.x * GROUP_KEYS + r * GROUP + threadIdx.x;
        const bool root = key < f.n_keys && L[key] == key;
        uint32_t all = 0u;
        const uint32_t id = next + group_exclusive_scan<GROUP / 64u>(root ? 1u : 0u, part, &all);
        next += all;
        if (!root) continue;
        uint32_t c[3];
        voxel_of(f, key, c);
        uint32_t* rec = (uint32_t*)(records + id);                     // first[3], lo[3], hi[3], reserved, voxels
        rec[0] = c[0]; rec[1] = c[1]; rec[2] = c[2];
        rec[3] = rec[4] = rec[5] = 0xffffffffu;
        rec[6] = rec[7] = rec[8] = 0u;
        rec[9] = 0u; rec[10] = 0u; rec[11] = 0u;
        L[key] = id | ROOT_FLAG;
    }
}

// Reads the roots' entries (flagged, written by no one here) and writes the others'.
__global__ __launch_bounds__(GROUP) void k_components_ids(Field f, uint32_t* L, vrc_component* records)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t r = 0; r < ROUNDS; ++r) {
        const uint32_t key = blockIdx.x * GROUP_KEYS + r * GROUP + threadIdx.x;      // whole waves pass or fail the bound
        if (key >= f.n_keys) return;
        const uint32_t v = L[key];
        uint32_t id = NONE;
        if (v != NONE) {
            if (v & ROOT_FLAG) id = v & ~ROOT_FLAG;
            else { id = L[v] & ~ROOT_FLAG; L[key] = id; }
        }
        uint32_t c[3];
        voxel_of(f, key, c);
        // one set of atomics per id present in the wave
        unsigned long long todo = __ballot(id != NONE);
        while (todo) {                                                               // wave-uniform
            const int leader = __ffsll((long long)todo) - 1;
            const uint32_t lid = __shfl(id, leader);
            const bool mine = id == lid;
            const unsigned long long same = __ballot(mine);
            todo &= ~same;
            uint32_t lo[3], hi[3];
            for (int a = 0; a < 3; ++a) { lo[a] = mine ? c[a] : 0xffffffffu; hi[a] = mine ? c[a] + 1u : 0u; }
            if (same & (same - 1ull)) {
                for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
            } else {
                for (int a = 0; a < 3; ++a) { lo[a] = __shfl(lo[a], leader); hi[a] = __shfl(hi[a], leader); }
            }
            if ((int)lane == leader) {
                vrc_component* rec = records + lid;
                atomicAdd((unsigned long long*)&rec->voxels, (unsigned long long)__popcll(same));
                for (int a = 0; a < 3; ++a) { atomicMin(&rec->lo[a], lo[a]); atomicMax(&rec->hi[a], hi[a]); }
            }
        }
    }
}

__global__ __launch_bounds__(GROUP) void k_components_strip(Field f, uint32_t* __restrict__ L)
{
    for (uint32_t r = 0; r < ROUNDS; ++r) {
        const uint32_t key = blockIdx.x * GROUP_KEYS + r * GROUP + threadIdx.x;
        if (key >= f.n_keys) return;
        const uint32_t v = L[key];
        if (v != NONE && (v & ROOT_FLAG)) L[key] = v & ~ROOT_FLAG;
    }
}

__global__ void k_labels_at(Field f, const uint32_t* __restrict__ L, uint64_t count, const uint32_t* __restrict__ xyz, uint32_t* __restrict__ ids)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    ids[i] = x < f.S && y < f.S && z < f.S ? L[key_of(f, x, y, z)] : NONE;
}

// A lane per key: the two halves of a wave's ballot are two words of K = { v : keep[id(v)] != 0 }.  The lane of a word's
// first key writes the word, whole, with a plain store: a word has one owner.
__global__ __launch_bounds__(GROUP) void k_labels_select(Field f, const uint32_t* __restrict__ L, const uint8_t* __restrict__ keep, uint32_t* __restrict__ dst, int op)
{
    const uint32_t key = blockIdx.x * GROUP + threadIdx.x;             // whole waves pass or fail the bound
    if (key >= f.n_keys) return;
    const uint32_t id = L[key];
    const bool in = id != NONE && keep[id] != 0;
    const unsigned long long both = __ballot(in);
    if (key & 31u) return;
    const uint32_t K = (uint32_t)(key & 32u ? both >> 32 : both);
    store_selected_word(dst, key >> 5, K, op);
}

Field field_of(uint32_t depth, int through)
{
    Field f;
    f.lg = depth - 1u;
    f.S = 1u << depth;
    f.n_keys = 1u << (3u * depth);
    f.flip = through ? 0xffffffffu : 0u;
    return f;
}

uint32_t groups_of(uint32_t depth)
{
    const uint32_t n_keys = 1u << (3u * depth);
    return (n_keys + GROUP_KEYS - 1u) / GROUP_KEYS;
}

}  // namespace

namespace vrc {

size_t components_scratch_bytes(uint32_t depth) { return ((size_t)groups_of(depth) + 1u) * 4u; }

uint32_t* components_total_slot(uint32_t* scratch, uint32_t depth) { return scratch + groups_of(depth); }

void components_roots_run(const uint32_t* medium, uint32_t depth, int connectivity, int through, const uint32_t* cells, uint32_t* labels, uint32_t* scratch,
                          hipStream_t st)
{
    const Field f = field_of(depth, through);
    const dim3 grid(groups_of(depth)), block(GROUP);
    hipLaunchKernelGGL(k_components_init, grid, block, 0, st, f, medium, labels);
    if (connectivity == 6) {
        if (cells) hipLaunchKernelGGL((k_components_merge<6, true>), grid, block, 0, st, f, medium, labels, cells);
        else hipLaunchKernelGGL((k_components_merge<6, false>), grid, block, 0, st, f, medium, labels, cells);
    } else {
        if (cells) hipLaunchKernelGGL((k_components_merge<26, true>), grid, block, 0, st, f, medium, labels, cells);
        else hipLaunchKernelGGL((k_components_merge<26, false>), grid, block, 0, st, f, medium, labels, cells);
    }
    hipLaunchKernelGGL(k_components_flatten, grid, block, 0, st, f, labels, scratch);
    // a slot <= the keys of a workgroup, the total at most 2^30
    hipLaunchKernelGGL(k_scan_slots<uint32_t>, dim3(1), dim3(SCAN_GROUP), 0, st, scratch, groups_of(depth), (uint32_t*)nullptr);
}

void components_ids_run(uint32_t depth, uint32_t* labels, const uint32_t* scratch, vrc_component* records, hipStream_t st)
{
    const Field f = field_of(depth, 0);
    const dim3 grid(groups_of(depth)), block(GROUP);
    hipLaunchKernelGGL(k_components_roots, grid, block, 0, st, f, labels, scratch, records);
    hipLaunchKernelGGL(k_components_ids, grid, block, 0, st, f, labels, records);
    hipLaunchKernelGGL(k_components_strip, grid, block, 0, st, f, labels);
}

void components_at_run(const uint32_t* labels, uint32_t depth, uint64_t n, const uint32_t* xyz, uint32_t* ids, hipStream_t st)
{
    hipLaunchKernelGGL(k_labels_at, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, field_of(depth, 0), labels, n, xyz, ids);
}

void components_select_run(const uint32_t* labels, uint32_t depth, const uint8_t* keep, uint32_t* dst, int op, hipStream_t st)
{
    const Field f = field_of(depth, 0);
    hipLaunchKernelGGL(k_labels_select, dim3((f.n_keys + GROUP - 1u) / GROUP), dim3(GROUP), 0, st, f, labels, keep, dst, op);
}

}  // namespace vrc
