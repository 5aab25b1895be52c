// vrc_fracture.hip -- the Voronoi cell of every voxel around a list of sites (include/vrc.h: vrc_fracture_label): which
// site is nearest, not how far it is.  cell(p) = the index i of an in-volume site that minimises (|p - s_i|^2, i)
// lexicographically.  The field is dense, [(x*S + y)*S + z], one uint32 index per voxel, VRC_NO_COMPONENT = "none"; the
// passes work in place on it, one kernel each on one stream; no workgroup waits for another and no float takes part.
//
//   scatter  k_fracture_scatter: the field starts as "none"; a thread per site writes its index at the site's voxel with a
//            32-bit vector atomicMin, so duplicated coordinates resolve to the lowest index whatever the schedule, and leaves
//            the site's coordinates packed in the SITE TABLE, (x << 20) | (y << 10) | z, one word per site.
//   z        k_fracture_z: in a column every site has partial distance 0, so the nearest site of a voxel is the nearest
//            marker below or above it.  A wave takes a column (64 / S columns below 64^3) into registers, 64 entries at a
//            time; a ballot per 64 entries says where the markers are, a count of leading / trailing zeros under the lane's
//            mask finds the nearest one in the lane's own 64, and two wave-uniform carries (one walk up, one walk down)
//            bring the nearest one of the other chunks.  The nearer wins, of two equally near the lower index.
//   y, x     k_fracture_minplus<1 / 0>: the lower-envelope stack of vrc_distance.hip's k_distance_minplus, carrying the
//            index.  After the z pass the entry at (x, j, z) names a site of column (x, j); after the y pass the entry at
//            (j, y, z) names a site of the plane x = j.  So the entry read at position j of a line IS a site whose
//            coordinate along the line is j, and its partial distance f follows from its other coordinates and the line's:
//            both come out of the site table.
//
// The stack entry is the site's index alone, one word, and (j, f) are recomputed from the table whenever an entry is
// read back.  The alternative, a two-word entry (f << 10 | j, index), would still need the table (or a second dense field)
// to get f for the entries of the 4-byte cell field, would double the LDS of the in-LDS variant to 64 KiB per workgroup at
// 128^3 (64 lanes x S entries x 8 bytes) and the device stacks to 512 MiB at 512^3; with one word the stacks are exactly
// those of the distance transform: in LDS up to 128^3 (64 x 128 x 4 bytes = 32 KiB per workgroup, five workgroups to a
// compute unit's 160 KiB), from 256^3 on in a device block sized by the lines in flight.  The price is a dependent 4-byte
// gather from the table per field entry read and per stack entry re-read (a pop, an advance of the second walk); the
// table is 4 bytes per site and stays in cache.
//
// TIES.  k_distance_minplus pops a parabola when crossover(a, b) >= crossover(b, q) and advances on next <= val.  Both are
// right for values and wrong for indices: a parabola that is lowest nowhere STRICTLY can still tie at an integer point and
// carry the lowest index.  Here a parabola is popped only on strict >: then it lies strictly above a or strictly above q at
// every point and can never attain the minimum, tied or not.  The crossovers along the stack are then non-decreasing, so at
// a point i the values of the entries fall (weakly) up to an entry K(i) and rise strictly behind it, K(i) only moves
// forward with i, and the entries that attain the minimum at i are a run that ends at K(i) -- any number of parabolas can
// meet in one point.  The second walk therefore restarts the index at its current entry for every i and, advancing while
// next <= val, takes the new index on < and the smaller index on ==.
// Doing this per pass is globally right: the sites that tie for an intermediate voxel of a line (same partial distance to
// it, and the same coordinate along every axis still to come, by the paragraph above) are equidistant from EVERY voxel of the
// later lines through it, so whichever of them is carried, the later passes see the same distances, and carrying the lowest
// index of them makes "the lowest index among the ties" of each pass compose to the lowest index among all nearest sites.
// The last pass applies max_d2: a least squared distance above it gives "none" (finite distances are below 2^22, so
// VRC_DISTANCE_NONE cuts nothing off).
//
// Measured on an MI355X at 512^3 on the FastNoise terrain (tools/bench_edit.py --fracture, profiles/edit/
// bench_fracture.json; the whole vrc_fracture_label call, device time by events, median of 5, A B A B in one run against
// vrc_volume_distance_field + vrc_volume_label_components of the same medium): 64 sites within radius 48 with the matching
// cut-off 16.30 ms next to 18.18 ms (0.90), 4096 sites over the whole volume 7.09 ms next to 18.01 ms (0.39; many small
// pieces label faster than the terrain's one).  The passes have not been timed apart.
#include "vrc_fracture.h"

namespace {

constexpr uint32_t NONE = VRC_NO_COMPONENT;
constexpr uint32_t GROUP = 256;               // lanes per workgroup of the scatter, the z pass and the piece cells
constexpr uint32_t LANES = 64;                // lines per workgroup of the min-plus passes: one wave
constexpr uint32_t LDS_STACK_MAX_DEPTH = 7;   // 64 x 128 x 4 bytes = 32 KiB
constexpr uint32_t WAVES_PER_CU = 8;          // lines in flight = compute units x 8 x 64
constexpr uint32_t MAX_CHUNKS = 16;           // 64-entry chunks of a column at 1024^3

__global__ __launch_bounds__(GROUP) void k_fracture_scatter(uint64_t n, const int32_t* __restrict__ sites, uint32_t depth, uint32_t* cells,
                                                            uint32_t* __restrict__ table)
{
    const uint64_t i = (uint64_t)blockIdx.x * GROUP + threadIdx.x;
    if (i >= n) return;
    const uint32_t S = 1u << depth;
    const uint32_t x = (uint32_t)sites[3 * i], y = (uint32_t)sites[3 * i + 1], z = (uint32_t)sites[3 * i + 2];   // below 0 wraps to above S
    const bool in = x < S && y < S && z < S;
    table[i] = in ? (x << 20) | (y << 10) | z : 0u;                  // a site outside is never named by the field
    if (in) atomicMin(&cells[(((size_t)x << depth | y) << depth) | z], (uint32_t)i);
}

// A unit = W = max(S, 64) consecutive entries: a column from 64^3 on, 64 / S whole columns below.  A wave per unit.
__global__ __launch_bounds__(GROUP) void k_fracture_z(uint32_t* cells, uint32_t depth)
{
    const uint32_t S = 1u << depth, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t W = S < 64u ? 64u : S, chunks = W >> 6, units = (1u << (3u * depth)) / W;      // 8^depth >= 64
    // the lanes of my own column
    const unsigned long long seg = S >= 64u ? ~0ull : ((1ull << S) - 1ull) << (lane & ~(S - 1u));
    for (uint32_t u = blockIdx.x * (GROUP / 64u) + wave; u < units; u += gridDim.x * (GROUP / 64u)) {      // uniform for the wave
        uint32_t* col = cells + (size_t)u * W;
        uint32_t v[MAX_CHUNKS], below[MAX_CHUNKS], below_at[MAX_CHUNKS];
        unsigned long long has[MAX_CHUNKS];
        // the whole unit is read before any of it is written: the pass is in place
#pragma unroll
        for (uint32_t ch = 0; ch < MAX_CHUNKS; ++ch) {
            v[ch] = NONE; has[ch] = 0ull;
            if (ch < chunks) {
                v[ch] = col[ch * 64u + lane];
                has[ch] = __ballot(v[ch] != NONE);
            }
        }
        // upwards: the nearest marker at or below every entry; (ci, cat) = the last marker of the chunks passed
        uint32_t ci = NONE, cat = 0u;
#pragma unroll
        for (uint32_t ch = 0; ch < MAX_CHUNKS; ++ch) {
            if (ch < chunks) {
                const unsigned long long m = has[ch] & seg & (~0ull >> (63u - lane));
                const uint32_t p = m ? 63u - (uint32_t)__clzll((long long)m) : lane;
                const uint32_t got = __shfl(v[ch], (int)p);
                below[ch] = m ? got : ci;
                below_at[ch] = m ? ch * 64u + p : cat;
                if (has[ch]) {
                    const uint32_t top = 63u - (uint32_t)__clzll((long long)has[ch]);
                    ci = __shfl(v[ch], (int)top); cat = ch * 64u + top;
                }
            }
        }
        // downwards: the nearest marker at or above, the choice between the two, and the store
        ci = NONE; cat = 0u;
#pragma unroll
        for (uint32_t c = 0; c < MAX_CHUNKS; ++c) {
            const uint32_t ch = MAX_CHUNKS - 1u - c;
            if (ch < chunks) {
                const unsigned long long m = has[ch] & seg & (~0ull << lane);
                const uint32_t p = m ? (uint32_t)__ffsll((long long)m) - 1u : lane;
                const uint32_t got = __shfl(v[ch], (int)p);
                const uint32_t above = m ? got : ci, above_at = m ? ch * 64u + p : cat;
                const uint32_t at = ch * 64u + lane;
                uint32_t out = below[ch];
                if (above != NONE) {
                    if (out == NONE) out = above;
                    else {
                        const uint32_t db = at - below_at[ch], da = above_at - at;
                        if (da < db || (da == db && above < out)) out = above;
                    }
                }
                col[at] = out;
                if (has[ch]) {
                    const uint32_t low = (uint32_t)__ffsll((long long)has[ch]) - 1u;
                    ci = __shfl(v[ch], (int)low); cat = ch * 64u + low;
                }
            }
        }
    }
}

// what a table word says to a line: the site's coordinate along the line, and its squared distance to the line
template <int AXIS>
__device__ __forceinline__ void site_on_line(uint32_t t, int32_t pa, int32_t pz, int32_t& j, int32_t& f)
{
    const int32_t sx = (int32_t)(t >> 20), sy = (int32_t)((t >> 10) & 1023u), sz = (int32_t)(t & 1023u);
    const int32_t dz = pz - sz;
    if (AXIS == 1) { j = sy; f = dz * dz; }
    else { const int32_t dy = pa - sy; j = sx; f = dy * dy + dz * dz; }
}

// AXIS 1: the lines along y, line l = x * S + z.  AXIS 0: the lines along x, l = y * S + z, the last pass.
template <int AXIS, bool IN_LDS>
__global__ __launch_bounds__(LANES) void k_fracture_minplus(uint32_t* cells, uint32_t depth, const uint32_t* __restrict__ table, uint32_t* stacks, uint32_t max_d2)
{
    extern __shared__ uint32_t lds_stacks[];
    const uint32_t S = 1u << depth, lines = S * S, lane = threadIdx.x;
    const uint32_t sh = AXIS == 1 ? depth : 2u * depth;          // log2 of the step along the line
    uint32_t* stk;                                               // entry k of this lane: stk[k * LANES], a site index
    if (IN_LDS) stk = lds_stacks + lane;
    else stk = stacks + (size_t)blockIdx.x * LANES * S + lane;
    for (uint32_t l0 = blockIdx.x * LANES; l0 < lines; l0 += gridDim.x * LANES) {
        const uint32_t l = l0 + lane;
        if (l >= lines) break;                                   // 4^3 only: 16 lines
        const uint32_t base = AXIS == 1 ? (((l >> depth) << (2u * depth)) | (l & (S - 1u))) : l;
        const int32_t pa = (int32_t)(l >> depth), pz = (int32_t)(l & (S - 1u));      // AXIS 0: the voxel is (i, pa, pz)
        uint32_t* line = cells + base;
        // first walk: the parabolas that attain the lower envelope somewhere, left to right; (va, Fa) and (vb, Fb) mirror
        // the two topmost entries, F = f + v^2
        uint32_t top = 0u;
        int32_t va = 0, Fa = 0, vb = 0, Fb = 0;
        for (uint32_t j0 = 0; j0 < S; j0 += 4u) {
            uint32_t s4[4], t4[4];
            for (uint32_t u = 0; u < 4u; ++u) s4[u] = line[(size_t)(j0 + u) << sh];
            for (uint32_t u = 0; u < 4u; ++u) t4[u] = s4[u] != NONE ? table[s4[u]] : 0u;
            for (uint32_t u = 0; u < 4u; ++u) {
                if (s4[u] == NONE) continue;
                int32_t q, f;
                site_on_line<AXIS>(t4[u], pa, pz, q, f);         // q == j0 + u
                const int32_t Fq = f + q * q;
                // b attains the minimum nowhere only if crossover(a, b) > crossover(b, q), STRICTLY:
                // (Fb - Fa) / (vb - va) > (Fq - Fb) / (q - vb), both denominators positive
                while (top >= 2u && (int64_t)(Fb - Fa) * (q - vb) > (int64_t)(Fq - Fb) * (vb - va)) {
                    --top;
                    vb = va; Fb = Fa;
                    if (top >= 2u) {
                        site_on_line<AXIS>(table[stk[(top - 2u) * LANES]], pa, pz, va, Fa);
                        Fa += va * va;
                    }
                }
                stk[top * LANES] = s4[u];
                va = vb; Fa = Fb; vb = q; Fb = Fq;
                ++top;
            }
        }
        // second walk: at i, the lowest index among the entries that attain the envelope's value; the pointer only moves
        // forward
        uint32_t k = 0u, sc = NONE, sn = NONE;
        int32_t vc = 0, fc = 0, vn = 0, fn = 0;
        if (top) { sc = stk[0]; site_on_line<AXIS>(table[sc], pa, pz, vc, fc); }
        if (top > 1u) { sn = stk[LANES]; site_on_line<AXIS>(table[sn], pa, pz, vn, fn); }
        for (uint32_t i = 0; i < S; ++i) {
            uint32_t out = NONE;
            if (top) {
                int32_t d = (int32_t)i - vc;
                uint32_t val = (uint32_t)(fc + d * d);
                out = sc;                                        // the ties of i - 1 lie behind: the run of i starts here
                while (k + 1u < top) {
                    d = (int32_t)i - vn;
                    const uint32_t next = (uint32_t)(fn + d * d);
                    if (next > val) break;
                    out = next < val || sn < out ? sn : out;
                    ++k; vc = vn; fc = fn; sc = sn; val = next;
                    if (k + 1u < top) { sn = stk[(k + 1u) * LANES]; site_on_line<AXIS>(table[sn], pa, pz, vn, fn); }
                }
                if (AXIS == 0 && val > max_d2) out = NONE;
            }
            line[(size_t)i << sh] = out;
        }
    }
}

__global__ __launch_bounds__(GROUP) void k_fracture_piece_cells(const vrc_component* __restrict__ records, uint64_t count, const uint32_t* __restrict__ cells,
                                                                uint32_t depth, uint32_t* __restrict__ piece_cells)
{
    const uint64_t id = (uint64_t)blockIdx.x * GROUP + threadIdx.x;
    if (id >= count) return;
    const uint32_t* c = records[id].first;
    piece_cells[id] = cells[(((size_t)c[0] << depth | c[1]) << depth) | c[2]];
}

uint32_t minplus_groups(uint32_t depth, int cu_count)
{
    const uint32_t lines = 1u << (2u * depth);
    const uint32_t want = (lines + LANES - 1u) / LANES, cap = (uint32_t)(cu_count > 0 ? cu_count : 1) * WAVES_PER_CU;
    return want < cap ? want : cap;
}

size_t table_bytes(uint64_t n_sites) { return ((size_t)n_sites * 4u + 15u) & ~(size_t)15u; }

}  // namespace

namespace vrc {

size_t fracture_scratch_bytes(uint32_t depth, int cu_count, uint64_t n_sites)
{
    const size_t stacks = depth > LDS_STACK_MAX_DEPTH ? ((size_t)minplus_groups(depth, cu_count) * LANES * 4u) << depth : 0u;
    return table_bytes(n_sites) + stacks;
}

void fracture_cells_run(const int32_t* sites, uint64_t n_sites, uint32_t depth, uint32_t max_d2, int cu_count, uint32_t* cells, uint32_t* scratch,
                        hipStream_t st)
{
    uint32_t* table = scratch;
    uint32_t* stacks = scratch + table_bytes(n_sites) / 4u;
    (void)hipMemsetAsync(cells, 0xff, (size_t)4u << (3u * depth), st);
    hipLaunchKernelGGL(k_fracture_scatter, dim3((uint32_t)((n_sites + GROUP - 1u) / GROUP)), dim3(GROUP), 0, st, n_sites, sites, depth, cells, table);
    const uint32_t S = 1u << depth, units = (1u << (3u * depth)) / (S < 64u ? 64u : S);
    uint32_t z_groups = (units + GROUP / 64u - 1u) / (GROUP / 64u);
    const uint32_t z_cap = (uint32_t)(cu_count > 0 ? cu_count : 1) * 16u;
    if (z_groups > z_cap) z_groups = z_cap;
    hipLaunchKernelGGL(k_fracture_z, dim3(z_groups), dim3(GROUP), 0, st, cells, depth);
    const dim3 grid(minplus_groups(depth, cu_count)), block(LANES);
    if (depth <= LDS_STACK_MAX_DEPTH) {
        const size_t lds = ((size_t)LANES * 4u) << depth;
        hipLaunchKernelGGL((k_fracture_minplus<1, true>), grid, block, lds, st, cells, depth, table, nullptr, max_d2);
        hipLaunchKernelGGL((k_fracture_minplus<0, true>), grid, block, lds, st, cells, depth, table, nullptr, max_d2);
    } else {
        hipLaunchKernelGGL((k_fracture_minplus<1, false>), grid, block, 0, st, cells, depth, table, stacks, max_d2);
        hipLaunchKernelGGL((k_fracture_minplus<0, false>), grid, block, 0, st, cells, depth, table, stacks, max_d2);
    }
}

void fracture_piece_cells_run(const vrc_component* records, uint64_t count, const uint32_t* cells, uint32_t depth, uint32_t* piece_cells, hipStream_t st)
{
    hipLaunchKernelGGL(k_fracture_piece_cells, dim3((uint32_t)((count + GROUP - 1u) / GROUP)), dim3(GROUP), 0, st, records, count, cells, depth, piece_cells);
}

}  // namespace vrc
