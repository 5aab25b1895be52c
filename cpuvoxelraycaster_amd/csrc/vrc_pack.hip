// vrc_pack.hip -- an occupancy as a sparse tile stream and back (include/vrc.h: vrc_pack_volume, vrc_unpack_volume; the
// format, version 1, is described there and its arithmetic is vrc_pack.h's).
//
// A tile is E^3 bricks, E = 8 from 32^3 up: 64 rows (i, j) of 8 brick bytes that lie together along z.  A workgroup is ONE
// wave of 64 lanes and takes one tile, a lane one row with one 8-byte load or store; no workgroup waits for another.  At 4^3
// and 8^3 the whole volume is one tile whose bricks lie in memory in the order of their local index q, so a lane takes the
// four bricks of one occupancy word there (at 4^3 that word holds two brick rows) and 2 or 16 lanes work: those sizes have
// a branch of their own (E8 = false), as vrc_delta.hip's word_box and vrc_surface.hip's word_masks have.
//
// Pack is three passes on one stream:
//   1. count: a lane derives its row's slice of the `some` and `full` masks and its partial bricks, the wave reduces them with
//             shuffles to the tile's class and partial count.  Lane 0 writes two slots (is-mixed, partial count) and adds the
//             solid voxels with one 64-bit atomic; a full tile adds one to the full count.
//   2. scan:  one workgroup replaces both slot arrays by their exclusive prefixes (scan_slots): a mixed tile's rank and its
//             offset into D.
//   3. emit:  a tile that is not mixed leaves after reading two slots.  A mixed one reads its rows again, writes its B entry,
//             its masks -- the slices of 4 (8) lanes combined by shuffles into whole 32-bit stores -- and its partial bytes at
//             offset + the wave's exclusive scan of the lanes' counts.  A second small kernel writes the header, the class map
//             (a tile that is not mixed is full iff its first word is ~0; 16 lanes' fields combined into one store) and the
//             padding.  Nothing is patched from the host.
// Unpack checks before it writes:
//   1. classes: a lane per class field -- no class 3, nothing behind the last tile --, the class counts, the is-mixed slots;
//      then the rank scan.
//   2. masks: MW lanes per tile, one pair of mask words each, reduced across the MW lanes: full inside some, no bit at q >= K,
//      some != 0, full not whole, popcount(some & ~full) = the B entry; that count into the tile's slot; then the offset scan.
//   3. bytes: a lane per word of D: no 0x00 or 0xff below P, zero padding from P on, and the solid voxels.
//   4. write, launched only when the host found every first_* and count clean: a wave per tile stores all K brick bytes as
//      whole words.  A rank is used only below M and an offset into D only below P, whatever the stream claims.
// Tile, rank and byte counts stay below 2^28 and are 32-bit; the solid count is 64-bit.
#include "vrc_pack.h"

#include "vrc_group.h"

namespace {

using vrc::PackTotals;

constexpr uint32_t LANES = 64;                // one wave per workgroup in the per-tile kernels

// bit k set iff byte k of w is not 0
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w)
{
    const uint32_t h = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;   // bit 7 of every byte that is not 0
    return (h * 0x00204081u) >> 28;                                             // bits 7, 15, 23, 31 -> 0, 1, 2, 3
}
// bit k set iff byte k of w is 0xff
__device__ __forceinline__ uint32_t full_bytes(uint32_t w) { return ~nonzero_bytes(~w) & 0xfu; }

// the geometry of a lane's row in tile t: R bricks with local indices [R lane, R lane + R), at occupancy word `word`
template <bool E8>
struct Row {
    static constexpr uint32_t R = E8 ? 8u : 4u;
    bool active;
    uint32_t word;
};
template <bool E8>
__device__ __forceinline__ Row<E8> row_of(uint32_t depth, uint32_t t, uint32_t lane)
{
    Row<E8> r;
    if (E8) {
        const uint32_t lgn = depth - 1u, lgt = depth - 4u, tm = (1u << lgt) - 1u;      // n = 2^lgn bricks, T = 2^lgt tiles per axis
        const uint32_t tx = t >> (2u * lgt), ty = (t >> lgt) & tm, tz = t & tm;
        const uint32_t cx = 8u * tx + (lane >> 3), cy = 8u * ty + (lane & 7u);
        r.active = true;
        r.word = (((cx << lgn) + cy) << lgn) / 4u + 2u * tz;                           // the byte address / 4: n^3 / 4 < 2^25
    } else {
        r.active = lane < vrc::pack_tile_bricks(depth) / 4u;                           // 2 lanes at 4^3, 16 at 8^3
        r.word = lane;
    }
    return r;
}
// the row's brick bytes, 0 for a lane without a row; .y stays 0 where a row is four bricks
template <bool E8>
__device__ __forceinline__ uint2 row_load(const uint32_t* __restrict__ words, const Row<E8>& r)
{
    if (E8) return *(const uint2*)(words + r.word);
    return make_uint2(r.active ? words[r.word] : 0u, 0u);
}
template <bool E8>
__device__ __forceinline__ uint32_t some_slice(uint2 w) { return nonzero_bytes(w.x) | (E8 ? nonzero_bytes(w.y) << 4 : 0u); }
template <bool E8>
__device__ __forceinline__ uint32_t full_slice(uint2 w) { return full_bytes(w.x) | (E8 ? full_bytes(w.y) << 4 : 0u); }

// ---- pack ------------------------------------------------------------------------------------------------------------

template <bool E8>
__global__ __launch_bounds__(LANES) void k_pack_count(const uint32_t* __restrict__ words, uint32_t depth, uint32_t* __restrict__ slot_mixed,
                                                      uint32_t* __restrict__ slot_partial, PackTotals* __restrict__ totals)
{
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    const uint2 w = row_load<E8>(words, row_of<E8>(depth, t, lane));
    const uint32_t sm = some_slice<E8>(w), fl = full_slice<E8>(w);
    // some and full bricks of the tile <= 512 each, partial bricks <= 512, solid voxels <= 4096: two sums carry the four
    const uint32_t a = wave_sum((uint32_t)__popc(sm) | ((uint32_t)__popc(fl) << 16));
    const uint32_t b = wave_sum((uint32_t)__popc(sm & ~fl) | ((uint32_t)(__popc(w.x) + __popc(w.y)) << 16));
    if (lane != 0u) return;
    const uint32_t n_some = a & 0xffffu, n_full = a >> 16, n_partial = b & 0xffffu, solid = b >> 16;
    const bool mixed = n_some != 0u && n_full != vrc::pack_tile_bricks(depth);
    slot_mixed[t] = mixed ? 1u : 0u;
    slot_partial[t] = mixed ? n_partial : 0u;
    if (n_some != 0u && !mixed) atomicAdd(&totals->full, 1u);
    if (solid) atomicAdd(&totals->solid, (unsigned long long)solid);
}

// both slot arrays -> their exclusive prefixes with the totals behind them, and the totals.  One workgroup.
__global__ __launch_bounds__(SCAN_GROUP) void k_pack_scan(uint32_t* __restrict__ slot_mixed, uint32_t* __restrict__ slot_partial, uint32_t n_tiles,
                                                          PackTotals* __restrict__ totals)
{
    const uint32_t mixed = scan_slots(slot_mixed, n_tiles);             // a slot <= 1
    const uint32_t partial = scan_slots(slot_partial, n_tiles);         // a slot <= 512, the total <= 2^27
    if (threadIdx.x == 0) {
        slot_mixed[n_tiles] = mixed;
        slot_partial[n_tiles] = partial;
        totals->mixed = mixed;
        totals->partial = partial;
    }
}

struct PackHead {
    uint32_t depth, mixed, partial, full;
    unsigned long long length, solid;
};

// Header, class map and padding.  A lane per class field; 16 lanes' fields are one word.  grid * 256 >= 16 class_words.
template <bool E8>
__global__ __launch_bounds__(256) void k_pack_head(const uint32_t* __restrict__ words, PackHead h, const uint32_t* __restrict__ slot_mixed,
                                                   uint32_t* __restrict__ header, uint32_t* __restrict__ class_map, uint8_t* __restrict__ d_bytes)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, n_tiles = vrc::pack_tiles(h.depth);
    uint32_t cls = 0u;
    if (g < n_tiles) {
        if (slot_mixed[g + 1u] != slot_mixed[g]) cls = 2u;
        else cls = words[row_of<E8>(h.depth, g, 0u).word] == 0xffffffffu ? 1u : 0u;   // uniform tile: its first word says which
    }
    uint32_t v = cls << (2u * (g & 15u));
    for (int o = 1; o < 16; o <<= 1) v |= __shfl_xor(v, o);
    if ((g & 15u) == 0u && g / 16u < vrc::pack_class_words(h.depth)) class_map[g / 16u] = v;
    if (g < 16u) {
        const uint32_t head[16] = {vrc::PACK_MAGIC, vrc::PACK_VERSION, h.depth, n_tiles, h.mixed, h.partial, (uint32_t)h.length, (uint32_t)(h.length >> 32),
                                   (uint32_t)h.solid, (uint32_t)(h.solid >> 32), h.full, 0u, 0u, 0u, 0u, 0u};
        uint32_t mine = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) mine = g == k ? head[k] : mine;
        header[g] = mine;
    }
    if (g >= 16u && g < 19u) {                                        // at most three bytes of padding, a lane each
        const uint32_t at = h.partial + (g - 16u);
        if (at < ((h.partial + 3u) & ~3u)) d_bytes[at] = 0u;
    }
}

template <bool E8>
__global__ __launch_bounds__(LANES) void k_pack_emit(const uint32_t* __restrict__ words, uint32_t depth, const uint32_t* __restrict__ slot_mixed,
                                                     const uint32_t* __restrict__ slot_partial, uint32_t* __restrict__ counts,
                                                     uint32_t* __restrict__ masks, uint8_t* __restrict__ d_bytes)
{
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    const uint32_t rank = slot_mixed[t];
    if (slot_mixed[t + 1u] == rank) return;                             // uniform for the workgroup
    const uint32_t from = slot_partial[t], to = slot_partial[t + 1u];
    const uint2 w = row_load<E8>(words, row_of<E8>(depth, t, lane));
    const uint32_t sm = some_slice<E8>(w), fl = full_slice<E8>(w), ps = sm & ~fl;
    if (lane == 0u) counts[rank] = to - from;
    // masks: a lane's slice is R bits, 32 / R lanes make one word
    constexpr uint32_t R = Row<E8>::R, PER_WORD = 32u / R;
    const uint32_t mw = vrc::pack_mask_words(depth), sub = lane & (PER_WORD - 1u), mask_word = lane / PER_WORD;
    uint32_t vs = sm << (R * sub), vf = fl << (R * sub);
    for (uint32_t o = 1; o < PER_WORD; o <<= 1) {
        vs |= __shfl_xor(vs, o);
        vf |= __shfl_xor(vf, o);
    }
    uint32_t* mine = masks + (size_t)rank * 2u * mw;
    if (mask_word < mw) {
        if (sub == 0u) mine[mask_word] = vs;
        if (sub == 1u) mine[mw + mask_word] = vf;
    }
    // partial bytes, held to `to`: an edit between the passes cannot make the wave write beyond its tile's share
    uint32_t at = from + wave_exclusive_scan((uint32_t)__popc(ps));
#pragma unroll
    for (uint32_t k = 0; k < R; ++k)
        if (((ps >> k) & 1u) && at < to) d_bytes[at++] = (uint8_t)((k < 4u ? w.x : w.y) >> (8u * (k & 3u)));
}

// ---- unpack ----------------------------------------------------------------------------------------------------------

// A lane per class field.  grid * 256 >= 16 class_words.
__global__ __launch_bounds__(256) void k_unpack_classes(const uint32_t* __restrict__ class_map, uint32_t depth, uint32_t* __restrict__ slot_mixed,
                                                        PackTotals* __restrict__ totals)
{
    __shared__ uint32_t part[4];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, n_tiles = vrc::pack_tiles(depth);
    uint32_t cls = 0u;
    if (g / 16u < vrc::pack_class_words(depth)) cls = (class_map[g / 16u] >> (2u * (g & 15u))) & 3u;
    if (g < n_tiles ? cls == 3u : cls != 0u) atomicMin(&totals->first_class, g);
    if (g < n_tiles) slot_mixed[g] = cls == 2u ? 1u : 0u;
    const uint32_t sum = group_sum<4u>(g < n_tiles ? (cls == 2u ? 1u : 0u) | (cls == 1u ? 0x10000u : 0u) : 0u, part);     // <= 256 each
    if (threadIdx.x == 0) {
        if (sum & 0xffffu) atomicAdd(&totals->mixed, sum & 0xffffu);
        if (sum >> 16) atomicAdd(&totals->full, sum >> 16);
    }
}

// MW lanes per tile, lane j its words j of `some` and `full`.  slot_mixed is scanned.  M: the header's; a rank is used below it.
__global__ __launch_bounds__(256) void k_unpack_masks(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ masks, uint32_t depth, uint32_t M,
                                                      const uint32_t* __restrict__ slot_mixed, uint32_t* __restrict__ slot_partial,
                                                      PackTotals* __restrict__ totals)
{
    __shared__ uint32_t part[4];
    const uint32_t mw = vrc::pack_mask_words(depth), K = vrc::pack_tile_bricks(depth), n_tiles = vrc::pack_tiles(depth);
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, t = g / mw, j = g & (mw - 1u);
    uint32_t rank = 0u;
    bool mixed = false;
    if (t < n_tiles) {
        rank = slot_mixed[t];
        mixed = slot_mixed[t + 1u] != rank && rank < M;
    }
    uint32_t s = 0u, f = 0u;
    if (mixed) {
        const uint32_t* mine = masks + (size_t)rank * 2u * mw;
        s = mine[j];
        f = mine[mw + j];
    }
    // bit 0: full outside some, bit 1: a bit at q >= K (K = 8 alone is below a word), bit 2: some has a bit
    uint32_t flags = ((f & ~s) ? 1u : 0u) | ((K < 32u && ((s | f) >> K)) ? 2u : 0u) | (s ? 4u : 0u);
    uint32_t sums = (uint32_t)__popc(f) | ((uint32_t)__popc(s & ~f) << 16);                              // <= 512 each
    for (uint32_t o = 1; o < mw; o <<= 1) {
        flags |= __shfl_xor(flags, o);
        sums += __shfl_xor(sums, o);
    }
    const uint32_t n_full = sums & 0xffffu, n_partial = sums >> 16;
    uint32_t solid = 0u;
    if (j == 0u && t < n_tiles) {
        slot_partial[t] = mixed ? n_partial : 0u;
        if (mixed) {
            if (flags & 1u) atomicMin(&totals->first_subset, t);
            if (flags & 2u) atomicMin(&totals->first_range, t);
            if (!(flags & 4u)) atomicMin(&totals->first_empty, t);
            if (n_full == K) atomicMin(&totals->first_whole, t);
            if (counts[rank] != n_partial) atomicMin(&totals->first_count, t);
            solid = 8u * n_full;
        }
    }
    const uint32_t sum = group_sum<4u>(solid, part);                                                     // <= 256 * 4096
    if (threadIdx.x == 0 && sum) atomicAdd(&totals->solid, (unsigned long long)sum);
}

// A lane per word of D, grid-stride.  d_words: the section, d_at: its byte offset in the stream, P: the header's.
__global__ __launch_bounds__(256) void k_unpack_bytes(const uint32_t* __restrict__ d_words, uint32_t d_at, uint32_t P, PackTotals* __restrict__ totals)
{
    __shared__ uint32_t part[4];
    const uint32_t n_words = (P + 3u) / 4u;
    uint32_t solid = 0u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_words; i += gridDim.x * 256u) {
        const uint32_t w = d_words[i];
        const uint32_t inside = 4u * i + 4u <= P ? 0xfu : (1u << (P - 4u * i)) - 1u;                     // which bytes are D's, the rest padding
        const uint32_t nz = nonzero_bytes(w), ff = full_bytes(w);
        const uint32_t bad = (~nz | ff) & inside, pad = nz & ~inside & 0xfu;
        if (bad) atomicMin(&totals->first_byte, d_at + 4u * i + (uint32_t)(__ffs((int)bad) - 1));
        if (pad) atomicMin(&totals->first_padding, d_at + 4u * i + (uint32_t)(__ffs((int)pad) - 1));
        uint32_t keep = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) keep |= ((inside >> k) & 1u) ? 0xffu << (8u * k) : 0u;
        solid += (uint32_t)__popc(w & keep);
    }
    const uint32_t sum = group_sum<4u>(solid, part);
    if (threadIdx.x == 0 && sum) atomicAdd(&totals->solid, (unsigned long long)sum);
}

// A wave per tile, after every check has passed.  slot_mixed / slot_partial are scanned.
template <bool E8>
__global__ __launch_bounds__(LANES) void k_unpack_write(const uint32_t* __restrict__ class_map, const uint32_t* __restrict__ masks,
                                                        const uint8_t* __restrict__ d_bytes, uint32_t depth, uint32_t M, uint32_t P,
                                                        const uint32_t* __restrict__ slot_mixed, const uint32_t* __restrict__ slot_partial,
                                                        uint32_t* __restrict__ words)
{
    constexpr uint32_t R = Row<E8>::R;
    const uint32_t t = blockIdx.x, lane = threadIdx.x;
    const Row<E8> row = row_of<E8>(depth, t, lane);
    const uint32_t rank = slot_mixed[t];
    const bool mixed = slot_mixed[t + 1u] != rank && rank < M;          // uniform for the workgroup
    uint2 w = make_uint2(0u, 0u);
    if (!mixed) {
        const uint32_t cls = (class_map[t / 16u] >> (2u * (t & 15u))) & 3u;
        if (cls == 1u) w = make_uint2(0xffffffffu, 0xffffffffu);
    } else {
        const uint32_t mw = vrc::pack_mask_words(depth);
        const uint32_t* mine = masks + (size_t)rank * 2u * mw;
        uint32_t sm = 0u, fl = 0u;
        if (row.active) {                                               // bits [R lane, R lane + R) of either mask
            const uint32_t at = R * lane;
            sm = (mine[at / 32u] >> (at & 31u)) & ((1u << R) - 1u);
            fl = (mine[mw + at / 32u] >> (at & 31u)) & ((1u << R) - 1u);
        }
        const uint32_t ps = sm & ~fl;
        uint32_t at = slot_partial[t] + wave_exclusive_scan((uint32_t)__popc(ps));
#pragma unroll
        for (uint32_t k = 0; k < R; ++k) {
            uint32_t byte = ((fl >> k) & 1u) ? 0xffu : 0u;
            if ((ps >> k) & 1u) {
                byte = at < P ? d_bytes[at] : 0u;                       // below P whatever the counts claimed
                ++at;
            }
            if (k < 4u) w.x |= byte << (8u * k);
            else w.y |= byte << (8u * (k & 3u));
        }
    }
    if (!row.active) return;
    if (E8) *(uint2*)(words + row.word) = w;
    else words[row.word] = w.x;
}

PackTotals* totals_of(void* scratch) { return (PackTotals*)scratch; }
uint32_t* slot_mixed_of(void* scratch) { return (uint32_t*)((PackTotals*)scratch + 1); }
uint32_t* slot_partial_of(void* scratch, uint32_t depth) { return slot_mixed_of(scratch) + vrc::pack_tiles(depth) + 1u; }
uint32_t field_groups(uint32_t depth) { return (16u * vrc::pack_class_words(depth) + 255u) / 256u; }

void totals_reset(PackTotals* totals, hipStream_t st)
{
    (void)hipMemsetAsync(totals, 0xff, 32, st);                         // the eight first_*
    (void)hipMemsetAsync((uint8_t*)totals + 32, 0, sizeof(PackTotals) - 32u, st);
}

}  // namespace

namespace vrc {

size_t pack_scratch_bytes(uint32_t depth) { return sizeof(PackTotals) + 8u * ((size_t)pack_tiles(depth) + 1u); }

void pack_offsets_run(const uint32_t* words, uint32_t depth, void* scratch, hipStream_t st)
{
    const uint32_t nt = pack_tiles(depth);
    totals_reset(totals_of(scratch), st);
    if (depth >= 4u)
        hipLaunchKernelGGL(k_pack_count<true>, dim3(nt), dim3(LANES), 0, st, words, depth, slot_mixed_of(scratch), slot_partial_of(scratch, depth), totals_of(scratch));
    else
        hipLaunchKernelGGL(k_pack_count<false>, dim3(nt), dim3(LANES), 0, st, words, depth, slot_mixed_of(scratch), slot_partial_of(scratch, depth), totals_of(scratch));
    hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(SCAN_GROUP), 0, st, slot_mixed_of(scratch), slot_partial_of(scratch, depth), nt, totals_of(scratch));
}

void pack_emit_run(const uint32_t* words, uint32_t depth, const void* scratch, const PackTotals& totals, uint8_t* out, hipStream_t st)
{
    const uint32_t nt = pack_tiles(depth);
    const PackLayout l = pack_layout(depth, totals.mixed, totals.partial);
    const PackHead head = {depth, totals.mixed, totals.partial, totals.full, l.length, totals.solid};
    const uint32_t* sm = slot_mixed_of((void*)scratch);
    const uint32_t* sp = slot_partial_of((void*)scratch, depth);
    uint32_t *header = (uint32_t*)out, *class_map = (uint32_t*)(out + l.a), *counts = (uint32_t*)(out + l.b), *masks = (uint32_t*)(out + l.c);
    uint8_t* d_bytes = out + l.d;
    if (depth >= 4u) {
        hipLaunchKernelGGL(k_pack_head<true>, dim3(field_groups(depth)), dim3(256), 0, st, words, head, sm, header, class_map, d_bytes);
        if (totals.mixed) hipLaunchKernelGGL(k_pack_emit<true>, dim3(nt), dim3(LANES), 0, st, words, depth, sm, sp, counts, masks, d_bytes);
    } else {
        hipLaunchKernelGGL(k_pack_head<false>, dim3(field_groups(depth)), dim3(256), 0, st, words, head, sm, header, class_map, d_bytes);
        if (totals.mixed) hipLaunchKernelGGL(k_pack_emit<false>, dim3(nt), dim3(LANES), 0, st, words, depth, sm, sp, counts, masks, d_bytes);
    }
}

void unpack_check_run(const uint8_t* data, uint32_t depth, uint32_t M, uint32_t P, void* scratch, hipStream_t st)
{
    const uint32_t nt = pack_tiles(depth), mw = pack_mask_words(depth);
    const PackLayout l = pack_layout(depth, M, P);
    PackTotals* totals = totals_of(scratch);
    uint32_t *sm = slot_mixed_of(scratch), *sp = slot_partial_of(scratch, depth);
    totals_reset(totals, st);
    hipLaunchKernelGGL(k_unpack_classes, dim3(field_groups(depth)), dim3(256), 0, st, (const uint32_t*)(data + l.a), depth, sm, totals);
    hipLaunchKernelGGL(k_scan_slots<uint32_t>, dim3(1), dim3(SCAN_GROUP), 0, st, sm, nt, (uint32_t*)nullptr);           // a slot <= 1
    hipLaunchKernelGGL(k_unpack_masks, dim3((uint32_t)(((uint64_t)nt * mw + 255u) / 256u)), dim3(256), 0, st, (const uint32_t*)(data + l.b),
                       (const uint32_t*)(data + l.c), depth, M, sm, sp, totals);
    hipLaunchKernelGGL(k_scan_slots<uint32_t>, dim3(1), dim3(SCAN_GROUP), 0, st, sp, nt, &totals->partial);             // a slot <= 512
    const uint32_t d_words = (P + 3u) / 4u;
    if (d_words) {
        uint32_t groups = (d_words + 255u) / 256u;
        if (groups > 4096u) groups = 4096u;
        hipLaunchKernelGGL(k_unpack_bytes, dim3(groups), dim3(256), 0, st, (const uint32_t*)(data + l.d), (uint32_t)l.d, P, totals);
    }
}

void unpack_write_run(const uint8_t* data, uint32_t depth, uint32_t M, uint32_t P, const void* scratch, uint32_t* words, hipStream_t st)
{
    const uint32_t nt = pack_tiles(depth);
    const PackLayout l = pack_layout(depth, M, P);
    const uint32_t* sm = slot_mixed_of((void*)scratch);
    const uint32_t* sp = slot_partial_of((void*)scratch, depth);
    if (depth >= 4u)
        hipLaunchKernelGGL(k_unpack_write<true>, dim3(nt), dim3(LANES), 0, st, (const uint32_t*)(data + l.a), (const uint32_t*)(data + l.c), data + l.d, depth, M, P, sm, sp, words);
    else
        hipLaunchKernelGGL(k_unpack_write<false>, dim3(nt), dim3(LANES), 0, st, (const uint32_t*)(data + l.a), (const uint32_t*)(data + l.c), data + l.d, depth, M, P, sm, sp, words);
}

}  // namespace vrc
