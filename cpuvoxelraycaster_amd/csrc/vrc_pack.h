// vrc_pack.h -- the sparse tile stream of an occupancy (include/vrc.h: vrc_pack_*; format version 1): the format's arithmetic,
// shared by the host entry points (vrc_volume.hip) and the kernels (vrc_pack.hip), and the passes as vrc_volume.hip calls
// them.  The kernels know word arrays and byte streams only; volumes, their ordering and the staging of host memory stay
// with vrc_volume.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vrc {

constexpr uint32_t PACK_MAGIC = 0x50435256u;      // the bytes V R C P
constexpr uint32_t PACK_VERSION = 1u;
constexpr uint32_t PACK_HEADER_BYTES = 64u;

// ---- the format's arithmetic: one copy for host and device ---------------------------------------------------------
// depth 2..10; n = bricks per axis, E = tile edge in bricks, T = tiles per axis, NT = tiles, K = bricks per tile,
// MW = words per mask
__host__ __device__ constexpr uint32_t pack_n(uint32_t depth) { return 1u << (depth - 1u); }
__host__ __device__ constexpr uint32_t pack_edge(uint32_t depth) { return pack_n(depth) < 8u ? pack_n(depth) : 8u; }
__host__ __device__ constexpr uint32_t pack_tiles_per_axis(uint32_t depth) { return pack_n(depth) / pack_edge(depth); }
__host__ __device__ constexpr uint32_t pack_tiles(uint32_t depth)
{
    return pack_tiles_per_axis(depth) * pack_tiles_per_axis(depth) * pack_tiles_per_axis(depth);
}
__host__ __device__ constexpr uint32_t pack_tile_bricks(uint32_t depth) { return pack_edge(depth) * pack_edge(depth) * pack_edge(depth); }
__host__ __device__ constexpr uint32_t pack_mask_words(uint32_t depth) { return pack_tile_bricks(depth) < 32u ? 1u : pack_tile_bricks(depth) / 32u; }
__host__ __device__ constexpr uint32_t pack_class_words(uint32_t depth) { return (pack_tiles(depth) + 15u) / 16u; }

// where the sections of a stream with M mixed tiles and P partial bricks start, in bytes, and its length
struct PackLayout {
    uint64_t a, b, c, d, length;
};
__host__ __device__ inline PackLayout pack_layout(uint32_t depth, uint64_t M, uint64_t P)
{
    PackLayout l;
    l.a = PACK_HEADER_BYTES;
    l.b = l.a + 4ull * pack_class_words(depth);
    l.c = l.b + 4ull * M;
    l.d = l.c + 8ull * pack_mask_words(depth) * M;
    l.length = l.d + 4ull * ((P + 3ull) / 4ull);
    return l;
}
// the length with every tile mixed and every brick partial
inline uint64_t pack_bound_bytes(uint32_t depth)
{
    return pack_layout(depth, pack_tiles(depth), (uint64_t)pack_n(depth) * pack_n(depth) * pack_n(depth)).length;
}

// ---- the scratch block -----------------------------------------------------------------------------------------------
// What the passes reduce, at the front of the block.  pack_totals_reset puts every first_* to ~0 and the rest to 0.  A
// first_* is the least tile index (first_byte, first_padding: the least byte offset into the stream) that breaks its rule.
struct PackTotals {
    uint32_t first_class;             // a class field 3, or a set field behind the last tile
    uint32_t first_subset;            // full not inside some
    uint32_t first_range;             // a mask bit at q >= K
    uint32_t first_empty;             // some == 0
    uint32_t first_whole;             // full has all K bits
    uint32_t first_count;             // popcount(some & ~full) != the B entry
    uint32_t first_byte;              // a D byte 0x00 or 0xff
    uint32_t first_padding;           // a padding byte != 0
    uint32_t mixed;                   // class-2 tiles
    uint32_t full;                    // class-1 tiles
    uint32_t partial;                 // partial bricks: the sum of the per-tile counts
    uint32_t pad;
    unsigned long long solid;         // pack: the solid voxels; unpack: those of the mixed tiles (masks and D)
    unsigned long long pad2;
};
static_assert(sizeof(PackTotals) == 64, "the slots behind it start on a multiple of 16 bytes");

// Bytes of the block at `depth`: the totals, then two arrays of NT + 1 32-bit slots (is-mixed, partial count; after the
// scan their exclusive prefixes with the totals behind them): 8 (NT + 1) + 64, 2 MiB at depth 10 and 256 KiB at depth 9.
size_t pack_scratch_bytes(uint32_t depth);
// Passes 1 and 2 of a pack over the occupancy words: the totals (reset here first), each tile's rank among the mixed tiles
// and its offset into D.  Two kernels on `st`.
void pack_offsets_run(const uint32_t* words, uint32_t depth, void* scratch, hipStream_t st);
// Pass 3, after pack_offsets_run on the same stream: the whole stream -- header, class map, B, C, D and padding -- to
// out[0 .. length), 4-byte aligned, where `totals` is the host's copy of the block's front.  Two kernels on `st`.
void pack_emit_run(const uint32_t* words, uint32_t depth, const void* scratch, const PackTotals& totals, uint8_t* out, hipStream_t st);
// The device-side rules of a stream whose 64 header bytes passed the host's rules (M, P from the header, `bytes` its length):
// class count and rank scan, mask checks and offset scan, D and padding; the totals (reset here first) say what broke.  No
// kernel reads outside data[0 .. bytes) and none writes anything but the scratch.  Five kernels on `st`.
void unpack_check_run(const uint8_t* data, uint32_t depth, uint32_t M, uint32_t P, void* scratch, hipStream_t st);
// After unpack_check_run found nothing: every brick byte of the occupancy from the stream, a wave per tile.
void unpack_write_run(const uint8_t* data, uint32_t depth, uint32_t M, uint32_t P, const void* scratch, uint32_t* words, hipStream_t st);

}  // namespace vrc
